"""The analytic-signal handle on the MI355X: fourier_hip_hilbert_* through fourier_amd.Hilbert and hilbert / envelope on torch tensors,
against tests/hilbert_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_hilbert_emu.py (it also covers the argument
checks of the C ABI and the allocation-free property after reserve).

Sizes: 2048 and 4096 (the two smallest L1 x L2 shapes of the one-launch kernel), 32768 at f32 and 16384 at f64 (the largest), 1, 2, 255,
1000, 1031 (composed only: tiny, Bluestein, mixed-radix and prime inner plans); batch 5, and one batch of 1025 at N = 2048, more
workgroups than one per CU.  Inputs: seeded white Gaussian rows.  Tolerance, relative L2 over the whole output: 2 x base, base the
single-transform figure tests/test_gpu_real.py grants the route -- f32 2e-6 (4e-6 on a Bluestein plan), f64 1e-13 (1e-11 on a
Bluestein plan) -- because two transforms in T contribute; the same bound for the envelope (||z'| - |z|| <= |z' - z|).  Every figure is
printed before it is asserted.  Every case runs once."""
import numpy as np
import pytest

import hilbert_truth as truth
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


def has_fused(real, n):
    return n in (2048, 4096, 8192, 16384) or (n == 32768 and real == "f32")


def rows(torch, real, batch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(batch, n, dtype=dtypes(torch, real)[0], device="cuda", generator=g)


def run(torch, plan, x, what):
    """into a buffer whose output starts on an odd element with sentinels on both sides; checks them and that the input is unmodified"""
    rt, ct = dtypes(torch, plan.real)
    keep = x.clone()
    buf = torch.full((x.numel() + 3,), SENTINEL, dtype=ct if what == "analytic" else rt, device="cuda")
    out = buf[1:1 + x.numel()].view(x.shape)
    assert getattr(plan, what)(x, out=out) is out
    assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the output was written"
    assert torch.equal(x, keep), f"{what} modified its input"
    return out.cpu().numpy()


def note(real, what, route, n, err, bound):
    print(f"{what} {real} N={n} {route}: err {err:.3g} bound {bound:.3g}")
    assert err <= bound, (real, what, route, n, err, bound)


def check(torch, fa, real, n, batch):
    x = rows(torch, real, batch, n, 1000 * batch + n)
    xh = x.cpu().numpy()
    want = truth.analytic(xh)
    spectrum = np.linalg.norm(np.fft.fft(xh.astype(np.float64), axis=-1))
    plan = fa.Hilbert(n, real, 0)
    assert plan.describe().startswith("hilbert composed"), plan.describe()  # the default route
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        route = "one-launch" if fusion and has_fused(real, n) else "composed"
        assert plan.describe().startswith(f"hilbert {route}: "), plan.describe()
        bound = tol(plan, real)
        z, env = run(torch, plan, x, "analytic"), run(torch, plan, x, "envelope")
        note(real, "analytic", route, n, rel_l2(z, want), bound)
        note(real, "envelope", route, n, rel_l2(env, np.abs(want)), bound)
        note(real, "real part", route, n, rel_l2(z.real, xh), bound)
        if n >= 4:
            upper = np.linalg.norm(np.fft.fft(z.astype(np.complex128), axis=-1)[:, n // 2 + 1:])
            note(real, "upper half", route, n, upper / spectrum, bound)
        got[route] = z, env, bound
    if len(got) == 2:
        bound = 2 * max(got["one-launch"][2], got["composed"][2])
        for i, what in enumerate(("analytic", "envelope")):
            note(real, what, "routes", n, rel_l2(got["one-launch"][i], got["composed"][i]), bound)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes_on_both_routes(torch, fa, real):
    for n in (2048, 4096, 32768 if real == "f32" else 16384):
        check(torch, fa, real, n, 5)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(torch, fa, real):
    for n in (1, 2, 255, 1000, 1031):
        check(torch, fa, real, n, 5)
    plan = fa.Hilbert(32768, "f64", 0)  # no f64 kernel of that length
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("hilbert composed"), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_one_per_cu(torch, fa, real):
    check(torch, fa, real, 2048, 1025)


@pytest.mark.parametrize("fusion", [1, 0])
def test_f32_envelope_on_bases_that_are_only_4_byte_aligned(torch, fa, fusion):
    n, batch = 2048, 5
    x = rows(torch, "f32", batch, n, 5)
    holder = torch.zeros(batch * n + 1, dtype=torch.float32, device="cuda")
    shifted = holder[1:].view(batch, n)
    shifted.copy_(x)
    assert x.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 4
    plan = fa.Hilbert(n, "f32", 0)
    plan.set_option("fusion", fusion)
    aligned = plan.envelope(x)                     # a fresh tensor: 8-byte aligned
    assert aligned.data_ptr() % 8 == 0
    odd = run(torch, plan, shifted, "envelope")   # input and output on odd elements
    assert np.array_equal(aligned.cpu().numpy(), odd)
    note("f32", "envelope", f"fusion={fusion} unaligned", n, rel_l2(odd, truth.envelope(x.cpu().numpy())), tol(plan, "f32"))
    assert torch.equal(plan.analytic(shifted), plan.analytic(x))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_envelope_in_place(torch, fa, real):
    for n in (255, 2048):
        x = rows(torch, real, 5, n, 6)
        plan = fa.Hilbert(n, real, 0)
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            want = plan.envelope(x)
            y = x.clone()
            assert plan.envelope(y, out=y) is y and torch.equal(y, want), (real, n, fusion)


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
    for n in (255, 2048):
        x = rows(torch, real, 5, n, 7)
        whole = fx.Hilbert(n, real, 0)
        per = (n // 2 + 1 + n) * elem  # the half spectrum and the envelope's analytic signal of one row
        monkeypatch.setenv("FOURIER_HILBERT_SCRATCH_BYTES", str(2 * per + 8))
        try:
            small = fx.Hilbert(n, real, 0)
        finally:
            monkeypatch.delenv("FOURIER_HILBERT_SCRATCH_BYTES")
        assert small.describe().startswith("hilbert composed") and whole.describe().startswith("hilbert composed")
        want = truth.analytic(x.cpu().numpy())
        for what in ("analytic", "envelope"):
            a, b = run(torch, whole, x, what), run(torch, small, x, what)
            assert np.array_equal(a, b), (real, n, what)
            note(real, what, "composed chunks", n, rel_l2(b, want if what == "analytic" else np.abs(want)), tol(small, real))


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """analytic and envelope captured on a side stream as the first calls of a handle that reserved (they must not allocate), one linear
    graph, replayed twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, batch = 2048, 5
    xs = [rows(torch, "f32", batch, n, 20 + i) for i in range(3)]
    side = torch.cuda.Stream()
    other = fa.Hilbert(n, "f32", 0)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.analytic(xs[0])
        other.envelope(xs[0])
    side.synchronize()
    plan = fa.Hilbert(n, "f32", 0)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith("hilbert one-launch" if fusion else "hilbert composed"), plan.describe()
    plan.reserve(batch)
    torch.cuda.synchronize()
    dx = xs[0].clone()
    Z = torch.empty(batch, n, dtype=torch.complex64, device="cuda")
    E = torch.empty(batch, n, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.analytic(dx, out=Z)  # the first calls on this plan: captured
        plan.envelope(dx, out=E)
    for x in xs[1:]:
        dx.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eZ, eE = plan.analytic(x), plan.envelope(x)
        torch.cuda.synchronize()
        assert torch.equal(Z, eZ) and torch.equal(E, eE), fusion
        want = truth.analytic(x.cpu().numpy())
        assert rel_l2(Z.cpu().numpy(), want) <= tol(plan, "f32") and rel_l2(E.cpu().numpy(), np.abs(want)) <= tol(plan, "f32")


def test_torch_layer(torch, fa):
    for real in ("f32", "f64"):
        rt, ct = dtypes(torch, real)
        x = rows(torch, real, 6, 1000, 3).view(2, 3, 1000)
        plan = fa.Hilbert(1000, real, 0)
        # the module functions against the handle, bit for bit
        z, e = fa.hilbert(x), fa.envelope(x)
        assert z.shape == x.shape and z.dtype == ct and e.shape == x.shape and e.dtype == rt
        assert torch.equal(z, plan.analytic(x)) and torch.equal(e, plan.envelope(x))
        out = torch.empty(2, 3, 1000, dtype=ct, device="cuda")
        assert fa.hilbert(x, out=out) is out and torch.equal(out, z)
        y = x.clone()
        assert fa.envelope(y, out=y) is y and torch.equal(y, e)
        assert plan.analytic(x[0, 0]).shape == (1000,)
        # scipy's N: zero-padded and truncated rows
        xh = x.reshape(6, 1000).cpu().numpy()
        for N in (1200, 600):
            padded = np.zeros((6, N), xh.dtype)
            padded[:, :min(N, 1000)] = xh[:, :N]
            got = fa.hilbert(x, N=N)
            assert got.shape == (2, 3, N)
            assert rel_l2(got.reshape(6, N).cpu().numpy(), truth.analytic(padded)) <= tol(fa.Hilbert(N, real, 0), real), (real, N)
        # a non-last dim: the axis moved last, transformed, moved back
        t = rows(torch, real, 7, 300, 4).view(7, 3, 100)
        want = truth.analytic(t.cpu().numpy().transpose(1, 2, 0).reshape(300, 7)).reshape(3, 100, 7).transpose(2, 0, 1)
        got = fa.hilbert(t, dim=0)
        assert got.shape == t.shape and rel_l2(got.cpu().numpy(), want) <= tol(fa.Hilbert(7, real, 0), real)
        assert rel_l2(fa.envelope(t, dim=0).cpu().numpy(), np.abs(want)) <= tol(fa.Hilbert(7, real, 0), real)
        assert torch.equal(fa.hilbert(t.transpose(0, 2), dim=-1), got.transpose(0, 2))  # ... and a non-contiguous layout
        with pytest.raises(TypeError):
            plan.analytic(x, out=torch.empty(2, 3, 1000, dtype=ct))                # not on the device
        with pytest.raises(TypeError):
            plan.analytic(x, out=torch.empty(2, 3, 1000, dtype=rt, device="cuda"))  # not complex
        with pytest.raises(TypeError):
            plan.envelope(x, out=torch.empty(6, 1000, dtype=rt, device="cuda"))     # not the input's shape
        with pytest.raises(ValueError):
            plan.analytic(x[..., :999].contiguous())                                # the wrong last dimension
        with pytest.raises(TypeError):
            plan.envelope(x.to(torch.float64 if real == "f32" else torch.float32))
        with pytest.raises(fa.FourierError):
            plan.envelope(x.view(6, 1000)[:5], out=x.view(6, 1000)[1:])             # partial overlap
    x = rows(torch, "f32", 4, 1000, 9)
    for fn in (fa.hilbert, fa.envelope):
        with pytest.raises(TypeError):
            fn(x.cpu())
        with pytest.raises(TypeError):
            fn(x.to(torch.complex64))
        with pytest.raises(TypeError):
            fn(x, out=torch.empty(4, 999, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            fn(x[:, :0])
        with pytest.raises(ValueError):
            fn(x, dim=2)
    with pytest.raises(ValueError):
        fa.hilbert(x, N=0)
    with pytest.raises(ValueError):
        fa.Hilbert(0, "f32", 0)
