"""The non-uniform FFT handle on the MI355X: fourier_hip_nufft_* through fourier_amd.Nufft on device buffers against the product
library -- the cases of tests/nufft_cases.py, which the CPU twin tests/test_nufft_emu.py runs on the emulator build -- and the torch
layer (Nufft.to_modes / to_points, nufft1, nufft2).  The walks under the development switches run through
fourier_amd/lib/libfourier_experiments.so, the way tests/test_gpu_launch.py does.  GPU only: a captured graph replayed on a side
stream after reserve, and the torch layer.  Against tests/nufft_truth.py (the direct sums in f64 on the rounded inputs); measure,
bounds and shapes are stated in tests/nufft_cases.py.  Every figure is printed before it is asserted.  Every case runs once."""
import ctypes
import os

import numpy as np
import pytest

import nufft_cases as cases
import nufft_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

REALS = ["f32", "f64"]
TABLES = [0, 1]


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def fa(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    yield fourier_amd
    cases.report("gpu")


@pytest.fixture
def be(torch, fa, monkeypatch):
    return cases.DeviceBackend(fa, torch, monkeypatch)


@pytest.fixture
def bx(torch, fa, monkeypatch):
    """the backend bound to the experiments library for one test: it reads the development switches from the environment at create.
    A handle keeps the library it was created from."""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield cases.DeviceBackend(fa, torch, monkeypatch)
    _lib._lib = prev


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_signs_and_orders(be, real, table, n):
    eps = cases.TIGHT[real]
    cases.accuracy(be, real, n, eps, cases.points("random37", n, eps, real), table, batch=cases.RB + 1, what="sizes")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("name", cases.POINT_SETS)
def test_point_sets(be, real, table, name):
    for n in cases.sizes_for(name):
        eps = cases.TIGHT[real]
        cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, orders=(0,), what=name)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_widths_through_eps(be, real, table):
    for eps in cases.EPS[real]:
        # (the inputs of tests/test_nufft_emu.py's test of the same name, for its reasons)
        for n, name in ((101, "random37"), (100, "far"), (3, "first_cell"), (500, "random3000")):
            cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, signs=(-1,), orders=(0,), what=f"eps {eps} {name}")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("batch", [1, cases.RB - 1, cases.RB, cases.RB + 1, 2 * cases.RB + 1])
def test_batches(be, real, batch):
    eps = cases.TIGHT[real]
    for table in TABLES:
        cases.accuracy(be, real, 101, eps, cases.points("ties", 101, eps, real), table, batch=batch, signs=(1,), orders=(1,), what="batches")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_adjointness(be, real, table):
    for eps in cases.EPS[real]:
        for n, name in ((100, "random37"), (101, "last_cell"), (101, "first_cell"), (2, "ties"), (100, "below_pi")):
            cases.adjoint(be, real, n, eps, cases.points(name, n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
def test_the_two_routes_agree(be, real):
    for eps in cases.EPS[real]:
        cases.routes_agree(be, real, 101, eps, cases.points("random37", 101, eps, real))


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_orders_permutation_and_repetition_are_bit_exact(be, real, table):
    for n in (100, 101, 3):
        cases.orders_and_permutation(be, real, n, cases.TIGHT[real], table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_launch_walk(bx, real, table):
    eps = cases.TIGHT[real]
    for n, name in ((101, "random37"), (5, "random3000")):  # 3000 points: the interpolation beyond one workgroup
        x = cases.points(name, n, eps, real)
        for batch, items in ((2 * cases.RB + 1, 1), (3 * cases.RB, 2 * truth.grid_length(n, truth.width(eps, real))), (cases.RB + 2, 300)):
            cases.launch_walk(bx, real, n, eps, x, table, batch, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("rows", [2, 1])
def test_scratch_walk(bx, real, table, rows):
    eps = cases.TIGHT[real]
    for n in (100, 101):
        cases.scratch_walk(bx, real, n, eps, cases.points("random37", n, eps, real), table, rows)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_a_nan_stays_in_its_row(be, real, table):
    cases.nan_row(be, real, 101, cases.TIGHT[real], cases.points("random37", 101, cases.TIGHT[real], real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_set_points_again_replaces_the_points(be, real, table):
    cases.second_set_points_replaces(be, real, table)


@pytest.mark.parametrize("real", REALS)
def test_refusals_write_nothing(be, real):
    cases.refusals(be, real)


@pytest.mark.parametrize("table", TABLES)
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, be, table):
    n, eps, batch = 101, 1e-6, 6
    x = cases.points("random37", n, eps, "f32")
    g = torch.Generator(device="cuda").manual_seed(12)
    c0 = torch.randn((batch, len(x)), dtype=torch.complex64, device="cuda", generator=g)
    c1 = torch.randn((batch, len(x)), dtype=torch.complex64, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = cases.make(be, n, eps, "f32", table)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_points(x)
    with torch.cuda.stream(side):
        other.to_points(other.to_modes(c0))
    side.synchronize()
    plan = cases.make(be, n, eps, "f32", table)
    plan.set_points(x)
    plan.reserve(batch)
    torch.cuda.synchronize()
    d = c0.clone()
    f = torch.empty((batch, n), dtype=torch.complex64, device="cuda")
    back = torch.empty_like(c0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.to_modes(d, out=f)  # the first calls on this plan: captured, must not allocate
        plan.to_points(f, out=back)
    d.copy_(c1)
    graph.replay()
    torch.cuda.synchronize()
    ef = plan.to_modes(c1)
    eb = plan.to_points(ef)
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), ef.cpu().numpy()) and np.array_equal(back.cpu().numpy(), eb.cpu().numpy())
    want = truth.direct_modes(x, c1.cpu().numpy(), n, -1)
    err = rel_l2(f.cpu().numpy(), want)
    cases.note(be, "f32", table, f"graph replay on the new strengths w {truth.width(eps, 'f32')}", [(1, err, cases.terms("f32", n, eps, x, 1, c1.cpu().numpy(), -1, 0, want))])


@pytest.mark.parametrize("real", REALS)
def test_torch_layer(torch, fa, real):
    cdt = torch.complex64 if real == "f32" else torch.complex128
    eps = cases.TIGHT[real]
    n = 101
    x = cases.points("far", n, eps, real)
    g = torch.Generator(device="cuda").manual_seed(5)
    c = torch.randn((2, 3, len(x)), dtype=cdt, device="cuda", generator=g)
    f = torch.randn((2, 3, n), dtype=cdt, device="cuda", generator=g)
    c2, f2 = c.cpu().numpy().reshape(6, -1), f.cpu().numpy().reshape(6, n)
    want1, want2 = truth.direct_modes(x, c2, n, -1), truth.direct_points(x, f2, 1)
    bnd = cases.bound(real, n, eps, x, 1, c2, -1, 0, want1)
    for xs in (x, torch.from_numpy(x), torch.from_numpy(x).cuda(), x.astype(np.float64).tolist()):
        if isinstance(xs, list):
            with pytest.raises(TypeError):
                fa.nufft1(xs, c, n, eps)
            continue
        got = fa.nufft1(xs, c, n, eps)
        assert tuple(got.shape) == (2, 3, n)
        err = rel_l2(got.cpu().numpy().reshape(6, n), want1)
        print(f"nufft gpu {real} nufft1: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd
    got = fa.nufft2(x, f, eps)
    assert tuple(got.shape) == (2, 3, len(x))
    err = rel_l2(got.cpu().numpy().reshape(6, -1), want2)
    bnd = cases.bound(real, n, eps, x, 2, f2, 1, 0, want2)
    print(f"nufft gpu {real} nufft2: err {err:.3g} bound {bnd:.3g}")
    assert err <= bnd
    plan = fa.Nufft(n, eps, real, 0)
    plan.set_points(x)
    assert torch.equal(plan.to_modes(c), fa.nufft1(x, c, n, eps)) and torch.equal(plan.to_points(f), fa.nufft2(x, f, eps))
    out = torch.empty((2, 3, n), dtype=cdt, device="cuda")
    assert plan.to_modes(c, out=out) is out
    with pytest.raises(ValueError):
        plan.to_modes(f)  # the last dimension is not points()
    with pytest.raises(ValueError):
        plan.to_modes(c, isign=0)
    with pytest.raises(TypeError):
        plan.to_modes(c.real.contiguous())
