"""The N-D convolution handle on the MI355X: fourier_hip_convnd_* through fourier_amd.FftConvNd on device buffers against the product
library -- the cases of tests/convnd_cases.py, which the CPU twin tests/test_convnd_emu.py runs on the emulator build -- and the torch
layer (fftconvn, fftconv2, fftconvolven, fftconvolve2).  The walks under the development switches run through
fourier_amd/lib/libfourier_experiments.so, the way tests/test_gpu_launch.py does.  GPU only: repetition and power-of-two scaling bit
for bit, a captured graph replayed on new input as the first apply of a handle that reserved (it must not allocate), non-trailing
dims, and one moderate shape on each route whose leading axis runs a real axis route.  Against tests/convnd_truth.py (numpy in f64 on
the rounded inputs, scipy's direct sums for the linear modes); measure and bounds are stated in tests/convnd_cases.py.  Every figure
is printed before it is asserted.  Every case runs once."""
import ctypes
import os

import numpy as np
import pytest

import convnd_cases as cases
import convnd_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

REALS = ["f32", "f64"]


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
@pytest.mark.parametrize("shape", cases.MID_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_mid_kernel_edges_on_both_routes(be, real, shape):
    cases.mid_edges(be, real, shape)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_banks(be, real, fusion):
    cases.banks(be, real, fusion)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_windows(be, real, fusion):
    cases.windows(be, real, fusion)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_linear_modes_against_scipy(be, real, fusion):
    cases.linear_modes(be, real, fusion)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("items", [2, 1])
def test_scratch_walk(bx, real, fusion, items):
    for shape, windowed in (((4, 6), False), ((3, 8), True), ((2, 5, 6), True), ((4, 7), True)):
        if not fusion or cases.has_fused(shape):
            cases.scratch_walk(bx, real, shape, fusion, items, windowed)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_launch_walk(bx, real, fusion):
    for shape in ((4, 6), (2, 600), (2, 3, 2, 8)):  # (2, 600): a half spectrum beyond one workgroup, so the product sweep's N-D twin
        for batch in range(3, 8):
            cases.launch_walk(bx, real, shape, fusion, batch, True)


@pytest.mark.parametrize("real", REALS)
def test_argument_checks(be, real):
    cases.argument_checks(be, real)


def test_rank_1_and_rank_5_are_refused(fa):
    with pytest.raises(ValueError):
        fa.FftConvNd((16,), "f32", 0)
    from fourier_amd import _lib

    L = _lib.lib()
    assert not L.fourier_hip_convnd_create_float(1, (ctypes.c_size_t * 1)(16), 0)
    assert not L.fourier_hip_convnd_create_double(5, (ctypes.c_size_t * 5)(2, 2, 2, 2, 2), 0)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_repetition_and_power_of_two_scaling_are_bit_exact(be, real, fusion):
    rng = np.random.default_rng(31)
    for shape in ((5, 8), (3, 4, 10)):
        plan, route = cases.make(be, shape, real, fusion)
        x = cases.rand(rng, (4,) + shape, real)
        cases.set_filters(be, plan, cases.rand(rng, (3,) + tuple(min(3, n) for n in shape), real))
        y = cases.run(be, plan, x, first=1)
        assert cases.run(be, plan, x, first=1).tobytes() == y.tobytes(), (shape, route, "a repetition differs")
        for e in (40, -40):
            s = cases.ndt(real)(2.0) ** e
            assert cases.run(be, plan, x * s, first=1).tobytes() == (y * s).tobytes(), (shape, route, e)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_of_apply_after_reserve(torch, fa, be, fusion):
    shape, batch = (12, 16), 6
    g = torch.Generator(device="cuda").manual_seed(12)
    x0 = torch.randn((batch,) + shape, dtype=torch.float32, device="cuda", generator=g)
    x1 = torch.randn((batch,) + shape, dtype=torch.float32, device="cuda", generator=g)
    h = torch.randn((3, 3, 5), dtype=torch.float32, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other, _ = cases.make(be, shape, "f32", fusion)  # loads the kernels' code object (the first launch of a module is not capturable)
    with torch.cuda.stream(side):
        other.set_filters(h)
        other.apply(x0)
    side.synchronize()
    plan, route = cases.make(be, shape, "f32", fusion)
    plan.set_filters(h)
    plan.reserve(batch)
    torch.cuda.synchronize()
    d, o = x0.clone(), torch.empty_like(x0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.apply(d, 1, out=o)  # the first apply on this plan: captured, must not allocate
    d.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    eager = plan.apply(x1, 1)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), eager.cpu().numpy())
    cases.note(be, plan, "f32", route, "graph replay on the new items", rel_l2(o.cpu().numpy(), truth.circular(x1.cpu().numpy(), h.cpu().numpy(), shape, False, 1)))


@pytest.mark.parametrize("real", REALS)
def test_torch_layer_circular_and_non_trailing_dims(torch, fa, real):
    dt = torch.float32 if real == "f32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((3, 6, 8), dtype=dt, device="cuda", generator=g)
    h = torch.randn((2, 2, 3), dtype=dt, device="cuda", generator=g)
    tol = 3 * (2e-6 if real == "f32" else 1e-12)
    y = fa.fftconv2(x, h)
    err = rel_l2(y.cpu().numpy(), truth.circular(x.cpu().numpy(), h.cpu().numpy(), (6, 8)))
    print(f"convnd gpu {real} fftconv2: err {err:.3g} bound {tol:.3g}")
    assert err <= tol
    assert torch.equal(fa.fftconvn(x, h, (-2, -1)), y) and torch.equal(fa.fftconvn(x[0], h[0]), fa.fftconv2(x[:1], h[:1])[0])
    out = torch.empty_like(y)
    assert fa.fftconv2(x, h, out=out) is out and torch.equal(out, y)
    yc = fa.fftconv2(x, h, correlate=True)
    assert rel_l2(yc.cpu().numpy(), truth.circular(x.cpu().numpy(), h.cpu().numpy(), (6, 8), True)) <= tol
    # the transformed dimensions in front, and in another order: against the trailing result
    xt = x.permute(1, 2, 0).contiguous()                     # (6, 8, 3): dims (0, 1), the batch behind
    assert torch.equal(fa.fftconvn(xt, h, (0, 1)).permute(2, 0, 1), y)
    xs = x.permute(0, 2, 1).contiguous()                     # (3, 8, 6): dims (2, 1) = (rows, columns)
    assert torch.equal(fa.fftconvn(xs, h, (2, 1)).permute(0, 2, 1), y)
    with pytest.raises(ValueError):
        fa.fftconvn(x, h, (1, 1))
    with pytest.raises(TypeError):
        fa.fftconv2(x, h[0, 0])


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("correlate", [False, True])
def test_fftconvolve2_against_scipy(torch, fa, real, correlate):
    dt = torch.float32 if real == "f32" else torch.float64
    tol = 3 * (2e-6 if real == "f32" else 1e-12)
    g = torch.Generator(device="cuda").manual_seed(9)
    for a, k in cases.LINEAR:
        x = torch.randn((4,) + a, dtype=dt, device="cuda", generator=g)
        h = torch.randn((3,) + k, dtype=dt, device="cuda", generator=g)
        for mode in cases.MODES:
            y = fa.fftconvolve2(x, h, mode, correlate)
            want = truth.scipy_linear(x.cpu().numpy(), h.cpu().numpy(), mode, correlate)
            assert tuple(y.shape) == want.shape, (a, k, mode)
            err = rel_l2(y.cpu().numpy(), want)
            print(f"convnd gpu {real} fftconvolve2 a={a} k={k} {mode} correlate={correlate}: err {err:.3g} bound {tol:.3g}")
            assert err <= tol, (a, k, mode, correlate)
        assert torch.equal(fa.fftconvolven(x[0], h[0], "same", correlate), fa.fftconvolve2(x[:1], h[:1], "same", correlate)[0])
        exact = tuple(n + m - 1 for n, m in zip(a, k))  # a transform shape of the caller's, odd in the last dimension: the composed route
        assert rel_l2(fa.fftconvolve2(x, h, "full", correlate, shape=exact).cpu().numpy(),
                      truth.scipy_linear(x.cpu().numpy(), h.cpu().numpy(), "full", correlate)) <= tol
    with pytest.raises(ValueError):
        fa.fftconvolve2(x[:, :3].contiguous(), h, "valid")  # a < k in a dimension
    with pytest.raises(ValueError):
        fa.fftconvolve2(x, h, "full", shape=(4, 4))
    with pytest.raises(ValueError):
        fa.fftconvolve2(x, h, "circular")


@pytest.mark.parametrize("fusion", [1, 0])
def test_a_moderate_shape_runs_a_real_axis_route(be, fusion):
    """8 items of [256, 512] f32: the leading axis of 256 over 256 packed columns is the column tile or the transpose route"""
    shape = (256, 512)
    plan, route = cases.make(be, shape, "f32", fusion)
    assert "axis column tile" in plan.describe() or "axis transpose" in plan.describe(), plan.describe()
    rng = np.random.default_rng(37)
    x = cases.rand(rng, (8,) + shape, "f32")
    h = cases.rand(rng, (3, 5, 7), "f32")
    cases.set_filters(be, plan, h)
    y = cases.run(be, plan, x, first=1)
    cases.note(be, plan, "f32", route, "8 items of [256, 512]", rel_l2(y, truth.circular(x, h, shape, False, 1)))
