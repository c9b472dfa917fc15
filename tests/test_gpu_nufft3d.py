"""The 3-D non-uniform FFT handle on the MI355X: fourier_hip_nufft3d_* through fourier_amd.Nufft3d on device buffers against the
product library -- the cases of tests/nufft3d_cases.py, which the CPU twin tests/test_nufft3d_emu.py runs on the emulator build --
and the torch layer (Nufft3d.to_modes / to_points, nufft3d1, nufft3d2).  The walks under the development switches run through
fourier_amd/lib/libfourier_experiments.so, the way tests/test_gpu_nufft2d.py does.  GPU only: a captured graph replayed on a side
stream after reserve, and the torch layer.  Against tests/nufft3d_truth.py (the direct sums in f64 on the rounded inputs); measure,
bounds and shapes are stated in tests/nufft3d_cases.py.  Every figure is printed before it is asserted.  Every case runs once."""
import ctypes
import os

import numpy as np
import pytest

import nufft3d_cases as cases
import nufft3d_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

REALS = ["f32", "f64"]
TABLES = [0, 1]
RB = cases.RB
WALK_SIZES = ((16, 16, 16), (30, 4, 9), (20, 6, 21))


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
    cases.accuracy(be, real, n, eps, cases.points("random37", n, eps, real), table, batch=RB + 1, what="sizes")


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
        # (the inputs of tests/test_nufft3d_emu.py's test of the same name, for its reasons)
        for n, name in (((8, 9, 10), "random37"), ((3, 40, 5), "far"), ((2, 3, 4), "corner_cell"), ((16, 16, 16), "random3000")):
            cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, signs=(-1,), orders=(0,), what=f"eps {eps} {name}")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("batch", [1, RB - 1, RB, RB + 1, 2 * RB + 1])
def test_batches(be, real, batch):
    eps = cases.TIGHT[real]
    for table in TABLES:
        cases.accuracy(be, real, (8, 9, 10), eps, cases.points("ties", (8, 9, 10), eps, real), table, batch=batch, signs=(1,), orders=(1,), what="batches")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_adjointness(be, real, table):
    for eps in cases.EPS[real]:
        for n, name in (((8, 9, 10), "random37"), ((30, 4, 9), "corner_cell"), ((3, 40, 5), "wrap1"), ((2, 3, 4), "ties"), ((20, 6, 21), "wrap3")):
            cases.adjoint(be, real, n, eps, cases.points(name, n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
def test_the_two_routes_agree(be, real):
    for eps in cases.EPS[real]:
        cases.routes_agree(be, real, (8, 9, 10), eps, cases.points("random37", (8, 9, 10), eps, real))


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_orders_permutation_and_repetition_are_bit_exact(be, real, table):
    for n in ((8, 9, 10), (30, 4, 9), (2, 3, 4)):
        cases.orders_and_permutation(be, real, n, cases.TIGHT[real], table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_scaling_by_powers_of_two_is_exact(be, real, table):
    n, eps = (8, 9, 10), cases.TIGHT[real]
    cases.scaling(be, real, n, eps, cases.points("random37", n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_launch_walk(bx, real, table):
    eps = cases.TIGHT[real]
    for n, name in (((8, 9, 10), "random37"), ((2, 3, 4), "random3000")):  # 3000 points: the interpolation beyond one workgroup
        x = cases.points(name, n, eps, real)
        cells = int(np.prod(cases.grid(n, eps, real)))
        for batch, items in ((2 * RB + 1, 1), (3 * RB, 2 * cells), (RB + 2, 300)):
            cases.launch_walk(bx, real, n, eps, x, table, batch, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("items", [2, 1])
def test_scratch_walk(bx, real, table, items):
    eps = cases.TIGHT[real]
    for n in WALK_SIZES:  # f32 grids 32^3, 60 x 15 x 18 (two even lengths) and 40 x 15 x 45 (one: the accuracy bound only)
        cases.scratch_walk(bx, real, n, eps, cases.points("random37", n, eps, real), table, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_a_nan_stays_in_its_item(be, real, table):
    n, eps = (8, 9, 10), cases.TIGHT[real]
    cases.nan_item(be, real, n, eps, cases.points("random37", n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_no_result_depends_on_the_handles_history(be, real, table):
    cases.history(be, real, table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_one_mode_on_axis_3_agrees_with_the_2d_handle(be, real, table):
    cases.agrees_with_2d(be, real, table)


@pytest.mark.parametrize("real", REALS)
def test_refusals_write_nothing(be, real):
    cases.refusals(be, real)


@pytest.mark.parametrize("table", TABLES)
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, be, table):
    n, eps, batch = (8, 9, 10), 1e-6, 6
    x = cases.points("random37", n, eps, "f32")
    m = len(x[0])
    g = torch.Generator(device="cuda").manual_seed(12)
    c0 = torch.randn((batch, m), dtype=torch.complex64, device="cuda", generator=g)
    c1 = torch.randn((batch, m), dtype=torch.complex64, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = cases.make(be, n, eps, "f32", table)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_points(*x)
    with torch.cuda.stream(side):
        other.to_points(other.to_modes(c0))
    side.synchronize()
    plan = cases.make(be, n, eps, "f32", table)
    plan.set_points(*x)
    plan.reserve(batch)
    torch.cuda.synchronize()
    d = c0.clone()
    f = torch.empty((batch,) + n, dtype=torch.complex64, device="cuda")
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
    want = truth.direct_modes(x[0], x[1], x[2], c1.cpu().numpy(), n, -1)
    err = rel_l2(f.cpu().numpy(), want)
    cases.note(be, "f32", table, f"graph replay on the new strengths w {truth.width(eps, 'f32')}", [(1, err, cases.terms("f32", n, eps, x, 1, c1.cpu().numpy(), -1, 0, want))])


@pytest.mark.parametrize("real", REALS)
def test_torch_layer(torch, fa, real):
    cdt = torch.complex64 if real == "f32" else torch.complex128
    eps = cases.TIGHT[real]
    n = (8, 9, 10)
    x = cases.points("far", n, eps, real)
    m = len(x[0])
    g = torch.Generator(device="cuda").manual_seed(5)
    c = torch.randn((2, 3, m), dtype=cdt, device="cuda", generator=g)
    f = torch.randn((2, 3) + n, dtype=cdt, device="cuda", generator=g)
    c2, f2 = c.cpu().numpy().reshape(6, -1), f.cpu().numpy().reshape((6,) + n)
    want1, want2 = truth.direct_modes(x[0], x[1], x[2], c2, n, -1), truth.direct_points(x[0], x[1], x[2], f2, 1)
    bnd = cases.bound(real, n, eps, x, 1, c2, -1, 0, want1)
    for conv in (lambda v: v, torch.from_numpy, lambda v: torch.from_numpy(v).cuda(), lambda v: v.tolist()):
        xs = tuple(conv(v) for v in x)
        if isinstance(xs[0], list):
            with pytest.raises(TypeError):
                fa.nufft3d1(*xs, c, n, eps)
            continue
        got = fa.nufft3d1(*xs, c, n, eps)
        assert tuple(got.shape) == (2, 3) + n
        err = rel_l2(got.cpu().numpy().reshape((6,) + n), want1)
        print(f"nufft3d gpu {real} nufft3d1: err {err:.3g} bound {bnd:.3g}")
        assert err <= bnd
    got = fa.nufft3d2(*x, f, eps)
    assert tuple(got.shape) == (2, 3, m)
    err = rel_l2(got.cpu().numpy().reshape(6, -1), want2)
    bnd = cases.bound(real, n, eps, x, 2, f2, 1, 0, want2)
    print(f"nufft3d gpu {real} nufft3d2: err {err:.3g} bound {bnd:.3g}")
    assert err <= bnd
    plan = fa.Nufft3d(n, eps, real, 0)
    plan.set_points(*x)
    assert torch.equal(plan.to_modes(c), fa.nufft3d1(*x, c, n, eps)) and torch.equal(plan.to_points(f), fa.nufft3d2(*x, f, eps))
    out = torch.empty((2, 3) + n, dtype=cdt, device="cuda")
    assert plan.to_modes(c, out=out) is out
    with pytest.raises(ValueError):
        plan.to_modes(f)  # the last dimension is not points()
    with pytest.raises(ValueError):
        plan.to_points(c)  # the trailing dimensions are not the modes
    with pytest.raises(ValueError):
        plan.to_modes(c, isign=0)
    with pytest.raises(ValueError):
        plan.set_points(x[0], x[1], x[2][:-1])
    with pytest.raises(ValueError):
        fa.nufft3d2(*x, f[0, 0, 0])  # fewer than three mode dimensions
    with pytest.raises(TypeError):
        plan.to_modes(c.real.contiguous())
