"""The resampling handle on the MI355X: fourier_hip_resample_* through fourier_amd.Resample and resample on torch tensors, against
tests/resample_truth.py (the definition of include/fourier.h in f64 numpy on the rounded input).  The CPU twin is
tests/test_resample_emu.py (it also cross-checks the truth against scipy.signal.resample, and holds the small and odd shapes and the
allocation-free property after reserve); the argument checks of the C ABI are tests/test_resample_abi.py.

Shapes (N, M): (2048, 4096), (4096, 2048) -- one-launch inner plans; (48000, 44100), (44100, 48000) -- mixed-radix inner plans;
(1000, 1031), (1031, 1000) -- a Bluestein plan on one side and an odd length, composed only; (255, 256); (2048, 1024) with a batch of
1025, more workgroups than CUs.  Batch 5 unless stated.  Inputs: seeded white Gaussian rows; windows: seeded uniform values in
[0.5, 1.5].  Tolerance, relative L2 over the whole output: 2 x base, base the single-transform figure tests/test_gpu_real.py grants --
f32 2e-6 (4e-6 if either plan's describe names Bluestein), f64 1e-13 (1e-11 likewise) -- because two transforms in T contribute (the
rule of tests/test_gpu_hilbert.py); the window is bounded by 1.5 and adds one rounding, no allowance of its own.  Every figure is
printed before it is asserted.  Every case runs once."""
import numpy as np
import pytest

import resample_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 77.0


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
    return fourier_amd


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return 2 * base


def dtypes(torch, real):
    return (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)


def rows(torch, real, batch, n, seed, complex_rows=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(batch, n, dtype=dtypes(torch, real)[1 if complex_rows else 0], device="cuda", generator=g)


def window(torch, real, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(n, dtype=dtypes(torch, real)[0], device="cuda", generator=g) + 0.5


def routes(plan):
    """the routes of a handle as (name, "fusion" value)"""
    if not plan.real_input:
        return (("complex", 0),)
    if plan.size_in() % 2 == 0 and plan.size_out() % 2 == 0:
        return (("real fused untangle", 1), ("real composed", 0))
    return (("real composed", 0),)


def select(plan, name, fusion):
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith(f"resample {name}: "), plan.describe()


def run(torch, plan, x):
    """into a buffer whose output starts on an odd element with sentinels on both sides; checks them and that the input is unmodified"""
    keep = x.clone()
    count = x.numel() // plan.size_in() * plan.size_out()
    buf = torch.full((count + 3,), SENTINEL, dtype=x.dtype, device="cuda")
    out = buf[1:1 + count].view(x.shape[:-1] + (plan.size_out(),))
    assert plan.forward(x, out=out) is out
    assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the output was written"
    assert torch.equal(x, keep), "forward modified its input"
    return out.cpu().numpy()


def note(real, what, route, shape, err, bound):
    print(f"{what} {real} {shape[0]}->{shape[1]} {route}: err {err:.3g} bound {bound:.3g}")
    assert err <= bound, (real, what, route, shape, err, bound)


def check(torch, fa, real, n, m, complex_rows, batch=5, windowed=False, only=None):
    """every route of the shape (or the routes named in `only`) against the truth; the two real routes within twice the bound of each other"""
    x = rows(torch, real, batch, n, 1000 * n + m + batch, complex_rows)
    w = window(torch, real, n, n + m) if windowed else None
    want = truth.resample(x.cpu().numpy(), m, None if w is None else w.cpu().numpy())
    plan = fa.Resample(n, m, real, 0, real_input=not complex_rows)
    plan.set_window(w)
    assert plan.describe().startswith(f"resample {routes(plan)[0][0]}: "), plan.describe()  # the default: the fused route where it exists
    what = ("windowed " if windowed else "") + ("complex rows" if complex_rows else "real rows")
    got = {}
    for name, fusion in routes(plan):
        if only is not None and name not in only:
            continue
        select(plan, name, fusion)
        y = run(torch, plan, x)
        bound = tol(plan, real)
        note(real, what, name, (n, m), rel_l2(y, want), bound)
        got[name] = y, bound
    assert got
    if len(got) == 2:
        (a, ba), (b, bb) = got.values()
        note(real, what, "real routes", (n, m), rel_l2(a, b), 2 * max(ba, bb))
    return plan


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(2048, 4096), (4096, 2048)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_one_launch_inner_plans(torch, fa, real, shape):
    check(torch, fa, real, shape[0], shape[1], False)
    check(torch, fa, real, shape[0], shape[1], True)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(48000, 44100), (44100, 48000)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_mixed_radix_inner_plans(torch, fa, real, shape):
    check(torch, fa, real, shape[0], shape[1], False)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1000, 1031), (1031, 1000)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_bluestein_and_odd_length_stay_on_the_composed_route(torch, fa, real, shape):
    plan = check(torch, fa, real, shape[0], shape[1], False)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("resample real composed: ") and "bluestein" in plan.describe(), plan.describe()
    check(torch, fa, real, shape[0], shape[1], True)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_255_to_256(torch, fa, real):
    check(torch, fa, real, 255, 256, False)
    check(torch, fa, real, 255, 256, True)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_cus(torch, fa, real):
    check(torch, fa, real, 2048, 1024, False, batch=1025, only=("real fused untangle",))
    check(torch, fa, real, 2048, 1024, True, batch=1025)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_windowed(torch, fa, real):
    check(torch, fa, real, 4096, 2048, False, windowed=True)
    check(torch, fa, real, 4096, 2048, True, windowed=True)


@pytest.mark.parametrize("fusion", [1, 0])
def test_f32_real_rows_on_bases_that_are_only_4_byte_aligned(torch, fa, fusion):
    n, m, batch = 2048, 1024, 5
    x = rows(torch, "f32", batch, n, 5)
    holder = torch.zeros(batch * n + 1, dtype=torch.float32, device="cuda")
    shifted = holder[1:].view(batch, n)
    shifted.copy_(x)
    assert x.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 4
    plan = fa.Resample(n, m, "f32", 0)
    plan.set_option("fusion", fusion)
    aligned = plan.forward(x)                 # a fresh tensor: 8-byte aligned
    assert aligned.data_ptr() % 8 == 0
    odd = run(torch, plan, shifted)           # input and output on odd elements
    assert np.array_equal(aligned.cpu().numpy(), odd)
    note("f32", "real rows", f"fusion={fusion} unaligned", (n, m), rel_l2(odd, truth.resample(x.cpu().numpy(), m)), tol(plan, "f32"))


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test (tests/test_gpu_chunks.py): it reads the scratch bound from the
    environment at create.  A handle keeps the library it was created from."""
    import ctypes
    import os

    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(torch, fx, real, monkeypatch):
    """a handle created under a bound of two rows of scratch walks 5 rows in 3 chunks: bit-equal to a handle of the same library
    without the bound, and within tolerance of the truth"""
    elem = 8 if real == "f32" else 16
    for n, m in ((255, 256), (2048, 1024)):
        for complex_rows in (False, True):
            x = rows(torch, real, 5, n, 7, complex_rows)
            per = n * elem if complex_rows else (n // 2 + 1 + m // 2 + 1) * elem  # a row's spectrum, or its two half spectra
            whole = fx.Resample(n, m, real, 0, real_input=not complex_rows)
            monkeypatch.setenv("FOURIER_RESAMPLE_SCRATCH_BYTES", str(2 * per + 8))
            try:
                small = fx.Resample(n, m, real, 0, real_input=not complex_rows)
            finally:
                monkeypatch.delenv("FOURIER_RESAMPLE_SCRATCH_BYTES")
            want = truth.resample(x.cpu().numpy(), m)
            for name, fusion in routes(whole):
                select(whole, name, fusion)
                select(small, name, fusion)
                a, b = run(torch, whole, x), run(torch, small, x)
                assert np.array_equal(a, b), (real, n, m, name)
                note(real, "chunks", name, (n, m), rel_l2(b, want), tol(small, real))


@pytest.mark.parametrize("route", ["real fused untangle", "real composed", "complex"])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, route):
    """forward captured on a side stream as the first call of a handle that reserved (it must not allocate), one linear graph, replayed
    twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, m, batch = 2048, 1024, 5
    complex_rows = route == "complex"
    fusion = int(route == "real fused untangle")
    xs = [rows(torch, "f32", batch, n, 20 + i, complex_rows) for i in range(3)]
    side = torch.cuda.Stream()
    other = fa.Resample(n, m, "f32", 0, real_input=not complex_rows)  # loads the kernels' code objects (not capturable)
    select(other, route, fusion)
    with torch.cuda.stream(side):
        other.forward(xs[0])
    side.synchronize()
    plan = fa.Resample(n, m, "f32", 0, real_input=not complex_rows)
    select(plan, route, fusion)
    plan.reserve(batch)
    torch.cuda.synchronize()
    dx = xs[0].clone()
    Y = torch.empty(batch, m, dtype=dx.dtype, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(dx, out=Y)  # the first call on this plan: captured
    for x in xs[1:]:
        dx.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eY = plan.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(Y, eY), route
        note("f32", "graph replay", route, (n, m), rel_l2(Y.cpu().numpy(), truth.resample(x.cpu().numpy(), m)), tol(plan, "f32"))


def test_torch_layer(torch, fa):
    for real in ("f32", "f64"):
        rt, ct = dtypes(torch, real)
        x = rows(torch, real, 6, 1000, 3).view(2, 3, 1000)
        plan = fa.Resample(1000, 600, real, 0)
        # the module function against the handle, bit for bit
        y = fa.resample(x, 600)
        assert y.shape == (2, 3, 600) and y.dtype == rt and torch.equal(y, plan.forward(x))
        out = torch.empty(2, 3, 600, dtype=rt, device="cuda")
        assert fa.resample(x, 600, out=out) is out and torch.equal(out, y)
        assert plan.forward(x[0, 0]).shape == (600,)
        note(real, "module function", "real rows", (1000, 600), rel_l2(y.cpu().numpy(), truth.resample(x.cpu().numpy(), 600)), tol(plan, real))
        # a window: a handle of its own; the cached one stays unwindowed
        w = window(torch, real, 1000, 9)
        plan.set_window(w)
        yw = fa.resample(x, 600, window=w)
        assert torch.equal(yw, plan.forward(x)) and torch.equal(fa.resample(x, 600), y)
        note(real, "module function", "windowed", (1000, 600),
             rel_l2(yw.cpu().numpy(), truth.resample(x.cpu().numpy(), 600, w.cpu().numpy())), tol(plan, real))
        # a complex dtype
        z = rows(torch, real, 4, 300, 4, True)
        cplan = fa.Resample(300, 450, real, 0, real_input=False)
        yz = fa.resample(z, 450)
        assert yz.dtype == ct and yz.shape == (4, 450) and torch.equal(yz, cplan.forward(z))
        note(real, "module function", "complex rows", (300, 450), rel_l2(yz.cpu().numpy(), truth.resample(z.cpu().numpy(), 450)), tol(cplan, real))
        # a non-last dim: the axis moved last, transformed, moved back; and a non-contiguous layout
        t = rows(torch, real, 7, 300, 5).view(7, 3, 100)
        want = truth.resample(t.cpu().numpy().transpose(1, 2, 0).reshape(300, 7), 9).reshape(3, 100, 9).transpose(2, 0, 1)
        got = fa.resample(t, 9, dim=0)
        assert got.shape == (9, 3, 100) and got.is_contiguous()
        note(real, "module function", "dim=0", (7, 9), rel_l2(got.cpu().numpy(), want), tol(fa.Resample(7, 9, real, 0), real))
        assert torch.equal(fa.resample(t.transpose(0, 2), 9, dim=-1), got.transpose(0, 2))
        o = torch.empty(9, 3, 100, dtype=rt, device="cuda")
        assert fa.resample(t, 9, dim=0, out=o) is o and torch.equal(o, got)
        with pytest.raises(TypeError):
            plan.forward(x, out=torch.empty(2, 3, 600, dtype=rt))                  # not on the device
        with pytest.raises(TypeError):
            plan.forward(x, out=torch.empty(2, 3, 600, dtype=ct, device="cuda"))   # not the input's dtype
        with pytest.raises(TypeError):
            plan.forward(x, out=torch.empty(6, 600, dtype=rt, device="cuda"))      # not the input's leading shape
        with pytest.raises(ValueError):
            plan.forward(x[..., :999].contiguous())                                # the wrong last dimension
        with pytest.raises(TypeError):
            plan.forward(x.to(torch.float64 if real == "f32" else torch.float32))
        with pytest.raises(TypeError):
            plan.forward(x.to(ct))                                                 # complex rows on a real handle
        with pytest.raises(ValueError):
            plan.set_window(w[:999].contiguous())
        with pytest.raises(fa.FourierError):
            plan.forward(x.view(-1)[:1000], out=x.view(-1)[400:1000])             # overlap
        with pytest.raises(fa.FourierError):
            plan.set_option("fusion", 2)
    x = rows(torch, "f32", 4, 1000, 9)
    with pytest.raises(TypeError):
        fa.resample(x.cpu(), 500)
    with pytest.raises(TypeError):
        fa.resample(x.to(torch.int32), 500)
    with pytest.raises(TypeError):
        fa.resample(x, 500, out=torch.empty(4, 499, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        fa.resample(x, 500, window=torch.ones(1000, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fa.resample(x, 500, window=torch.ones(999, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        fa.resample(x[:, :0], 500)
    with pytest.raises(ValueError):
        fa.resample(x, 0)
    with pytest.raises(ValueError):
        fa.resample(x, 500, dim=2)
    with pytest.raises(ValueError):
        fa.Resample(0, 8, "f32", 0)
