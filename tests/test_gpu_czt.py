"""The chirp-z handle on the MI355X: fourier_hip_czt_* through fourier_amd.Czt and czt / zoom_fft on torch tensors, on the cases of
tests/czt_cases.py (shapes, parameter sets, tolerance: base x R, base f32 4e-6 / f64 1e-11) against tests/czt_truth.py (the exact-phase
direct sum in f64 on the rounded input).  The CPU twin is tests/test_czt_emu.py (it also covers the argument checks of the C ABI, the
allocation-free property after reserve and the 65536-point DFT identity, which the emulator runs in a fraction of a second).  Here in
addition: a batch of 1025 rows (more workgroups than one per CU), graph replay, and the torch layer.  Every figure is printed before it
is asserted.  Every case runs once."""
import numpy as np
import pytest

import czt_cases as cases
import czt_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def backend(torch):
    class Backend:
        device = 0

        @staticmethod
        def run(plan, x, first=1):
            """numpy rows -> the handle's output as numpy, written into a buffer that starts on element `first` with sentinels on both
            sides; checks them and that the input is unmodified"""
            dx = torch.from_numpy(x).cuda()
            keep = dx.clone()
            count = x.shape[0] * plan.points()
            buf = torch.full((count + first + 2,), cases.SENTINEL, dtype=dx.dtype if dx.is_complex() else torch.complex64 if plan.real == "f32" else torch.complex128,
                             device="cuda")
            out = buf[first:first + count].view(x.shape[0], plan.points())
            assert plan.transform(dx, out=out) is out
            assert torch.all(buf[:first] == cases.SENTINEL).item() and torch.all(buf[-2:] == cases.SENTINEL).item(), "an element beside the output was written"
            assert torch.equal(dx, keep), "transform modified its input"
            return out.cpu().numpy()

    return Backend


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("L", [2048, 4096])
def test_one_launch_shapes_on_both_routes(fa, backend, real, L):
    for n, m in cases.one_launch_shapes(L):
        cases.check(backend, fa, real, n, m)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_largest_one_launch_length_without_slack(fa, backend, real):
    L = cases.TOP[real]
    cases.check(backend, fa, real, L // 2, L // 2 + 1)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("L", [2048, 4096])
def test_real_input(fa, backend, real, L):
    for n, m in cases.real_shapes(L):
        cases.check(backend, fa, real, n, m, real_input=True)


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("n", [1800, 1031])
def test_f32_real_input_offset_by_one_real(torch, fa, fusion, n):
    """the scalar loads (an input that is only 4-byte aligned; n odd) against the paired ones: bit-equal to the aligned call"""
    m, batch = {1800: 249, 1031: 999}[n], 5
    xh = truth.rows(np.random.default_rng(5), batch, n, np.float32)
    x = torch.from_numpy(xh).cuda()
    holder = torch.zeros(batch * n + 1, dtype=torch.float32, device="cuda")
    shifted = holder[1:].view(batch, n)
    shifted.copy_(x)
    assert x.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 4
    plan = fa.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, "f32", True, 0)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith("czt one-launch" if fusion else "czt composed")
    aligned, odd = plan.transform(x), plan.transform(shifted)
    assert torch.equal(aligned, odd)
    cases.note(None, "f32", "zoom real offset", "one-launch" if fusion else "composed", (n, m),
               rel_l2(odd.cpu().numpy(), truth.czt(xh, m, 1.0, -0.1 / m, 1.0, 0.2)), cases.BASE["f32"])


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_one_per_cu(fa, backend, real):
    cases.check(backend, fa, real, 1024, 1025, batch=1025, sets=("zoom",))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, backend, real):
    for n, m in ((1, 1), (3, 5), (255, 1000)):
        cases.check(backend, fa, real, n, m)
    for n, m in ((1, 1), (3, 5)):  # a tiny plan has no convolution route: forward, product, inverse
        plan = fa.Czt(n, m, real=real, device=0)
        assert plan.describe().startswith("czt composed: forward, product, inverse: "), plan.describe()  # L < 2048: the default


def test_f32_fused_pass_convolution_at_2_to_the_16(fa, backend):
    res = cases.check(backend, fa, "f32", 20000, 20000, batch=3, sets=("zoom",), routes=(1,))
    assert set(res) == {("zoom", "composed")}  # "fusion" = 1 has no one-launch kernel at L = 2^16
    plan = fa.Czt(20000, 20000, real="f32", device=0)
    assert plan.describe().startswith("czt composed: conv fused passes: "), plan.describe()


def test_f64_above_its_largest_kernel_stays_composed(fa):
    plan = fa.Czt(10000, 10000, real="f64", device=0)  # L = 2^15: f32 has a one-launch kernel, f64 has none
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("czt composed: "), plan.describe()


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
def test_chunk_walk_equals_the_one_chunk_result(fx, backend, real, monkeypatch):
    """a handle created under a bound of two rows of scratch walks 5 rows in 3 chunks: bit-equal to a handle of the same library
    without the bound, and within tolerance of the truth"""
    n, m, L = 255, 1000, 2048
    x = truth.rows(np.random.default_rng(7), 5, n, cases.cdt(real))
    whole = fx.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, real, False, 0)
    per = L * (8 if real == "f32" else 16)  # the work row
    monkeypatch.setenv("FOURIER_CZT_SCRATCH_BYTES", str(2 * per + 8))
    try:
        small = fx.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, real, False, 0)
    finally:
        monkeypatch.delenv("FOURIER_CZT_SCRATCH_BYTES")
    for plan in (whole, small):
        plan.set_option("fusion", 0)
        assert plan.describe().startswith("czt composed"), plan.describe()
    a, b = backend.run(whole, x), backend.run(small, x)
    assert np.array_equal(a, b)
    cases.note(None, real, "zoom", "composed chunks", (n, m), rel_l2(b, truth.czt(x, m, 1.0, -0.1 / m, 1.0, 0.2)), cases.BASE[real])


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_after_reserve(torch, fa, fusion):
    """one transform captured on one stream as the first call of a handle that reserved (it must not allocate), replayed twice on new
    input contents: bit-equal to the eager call, and within tolerance of the truth"""
    n, m, batch = 1031, 999, 5
    pars = (1.0, -0.1 / m, 1.0, 0.2)
    xs = [torch.from_numpy(truth.rows(np.random.default_rng(20 + i), batch, n, np.complex64)).cuda() for i in range(3)]
    side = torch.cuda.Stream()
    other = fa.Czt(n, m, *pars, "f32", False, 0)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.transform(xs[0])
    side.synchronize()
    plan = fa.Czt(n, m, *pars, "f32", False, 0)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith("czt one-launch" if fusion else "czt composed"), plan.describe()
    plan.reserve(batch)
    torch.cuda.synchronize()
    dx = xs[0].clone()
    Z = torch.empty(batch, m, dtype=torch.complex64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.transform(dx, out=Z)  # the first call on this plan: captured
    for x in xs[1:]:
        dx.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = plan.transform(x)
        torch.cuda.synchronize()
        assert torch.equal(Z, eager), fusion
        cases.note(None, "f32", "zoom graph", f"fusion={fusion}", (n, m), rel_l2(Z.cpu().numpy(), truth.czt(x.cpu().numpy(), m, *pars)), cases.BASE["f32"])


def test_torch_layer(torch, fa):
    for real in ("f32", "f64"):
        rt, ct = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
        n, m = 300, 120
        xh = truth.rows(np.random.default_rng(3), 6, n, cases.cdt(real))
        x = torch.from_numpy(xh).cuda().view(2, 3, n)
        base = cases.BASE[real]
        # czt with scipy's argument forms: defaults (the DFT), m, complex w and a
        got = fa.czt(x)
        assert got.shape == (2, 3, n) and got.dtype == ct
        assert rel_l2(got.reshape(6, n).cpu().numpy(), np.fft.fft(xh.astype(np.complex128), axis=-1)) <= base
        w, a = np.exp(-2j * np.pi * 0.0007), np.exp(2j * np.pi * 0.11)
        got = fa.czt(x, m, w, a)
        want = truth.czt(xh, m, abs(w), np.angle(w) / (2 * np.pi), abs(a), np.angle(a) / (2 * np.pi))
        assert got.shape == (2, 3, m)
        err = rel_l2(got.reshape(6, m).cpu().numpy(), want)
        print(f"czt torch {real} complex w, a: err {err:.3g} bound {base:.3g}")
        assert err <= base
        # the handle cache returns the same object for equal parameters, and the result is the handle's, bit for bit
        from fourier_amd import fft as F

        key = (n, m, abs(complex(w)), float(np.angle(w) / (2 * np.pi)), abs(complex(a)), float(np.angle(a) / (2 * np.pi)), real, False, 0)
        plan = F._cached_plan(fa.Czt, *key)
        assert F._cached_plan(fa.Czt, *key) is plan
        assert torch.equal(plan.transform(x), got)
        out = torch.empty(2, 3, m, dtype=ct, device="cuda")
        assert fa.czt(x, m, w, a, out=out) is out and torch.equal(out, got)
        # real input
        r = x.real.contiguous()
        err = rel_l2(fa.czt(r, m, w, a).reshape(6, m).cpu().numpy(), truth.czt(xh.real, m, abs(w), np.angle(w) / (2 * np.pi), abs(a), np.angle(a) / (2 * np.pi)))
        print(f"czt torch {real} real input: err {err:.3g} bound {base:.3g}")
        assert err <= base
        # zoom_fft: fn as a scalar and as a pair, endpoint, fs
        for fn, fs, endpoint in ((0.5, 2, False), ((0.2, 0.3), 2, False), ((100.0, 180.0), 1000.0, True)):
            f1, f2 = (0.0, fn) if np.ndim(fn) == 0 else fn
            w_turns = -(f2 - f1) / (fs * ((m - 1) if endpoint else m))
            got = fa.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)
            err = rel_l2(got.reshape(6, m).cpu().numpy(), truth.czt(xh, m, 1.0, w_turns, 1.0, f1 / fs))
            print(f"zoom_fft torch {real} fn={fn} fs={fs} endpoint={endpoint}: err {err:.3g} bound {base:.3g}")
            assert err <= base
        # m = None: as many points as samples
        assert fa.zoom_fft(x, 0.5).shape == (2, 3, n)
        # a non-last dim: the axis moved last, transformed, moved back
        th = truth.rows(np.random.default_rng(4), 7, 300, cases.cdt(real)).reshape(7, 3, 100)
        t = torch.from_numpy(th).cuda()
        want = truth.czt(th.transpose(1, 2, 0).reshape(300, 7), 5, 1.0, -0.03, 1.0, 0.0).reshape(3, 100, 5).transpose(2, 0, 1)
        got = fa.czt(t, 5, np.exp(-2j * np.pi * 0.03), dim=0)
        assert got.shape == (5, 3, 100) and rel_l2(got.cpu().numpy(), want) <= base
        got = fa.zoom_fft(t, (0.0, 0.3), 5, dim=0)
        assert got.shape == (5, 3, 100) and rel_l2(got.cpu().numpy(), want) <= base
        assert torch.equal(fa.zoom_fft(t.transpose(0, 2), (0.0, 0.3), 5, dim=-1), got.transpose(0, 2))  # ... and a non-contiguous layout
        plan = fa.Czt(n, m, real=real, device=0)
        with pytest.raises(TypeError):
            plan.transform(x, out=torch.empty(2, 3, m, dtype=ct))                  # not on the device
        with pytest.raises(TypeError):
            plan.transform(x, out=torch.empty(2, 3, n, dtype=ct, device="cuda"))   # not (..., m)
        with pytest.raises(ValueError):
            plan.transform(x[..., :n - 1].contiguous())                            # the wrong last dimension
        with pytest.raises(TypeError):
            plan.transform(x.real.contiguous())                                    # reals into a handle of complex rows
        with pytest.raises(TypeError):
            fa.Czt(n, m, real=real, real_input=True, device=0).transform(x)        # ... and complex rows into a handle of reals
        with pytest.raises(TypeError):
            plan.transform(x.to(torch.complex128 if real == "f32" else torch.complex64))
        flat = torch.zeros(6 * n, dtype=ct, device="cuda")
        with pytest.raises(fa.FourierError):
            plan.transform(flat.view(6, n), out=flat[:6 * m].view(6, m))           # overlapping out
        assert plan.transform(x[:0]).shape == (0, 3, m)                            # batch 0: a no-op
    x = torch.zeros(4, 100, dtype=torch.complex64, device="cuda")
    for fn in (fa.czt, lambda t, **kw: fa.zoom_fft(t, 0.5, **kw)):
        with pytest.raises(TypeError):
            fn(x.cpu())
        with pytest.raises(TypeError):
            fn(x.real.to(torch.int32))
        with pytest.raises(TypeError):
            fn(x, out=torch.empty(4, 99, dtype=torch.complex64, device="cuda"))
        with pytest.raises(ValueError):
            fn(x[:, :0])
        with pytest.raises(ValueError):
            fn(x, dim=2)
    with pytest.raises(ValueError):
        fa.czt(x, 0)
    with pytest.raises(ValueError):
        fa.zoom_fft(x, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError):
        fa.zoom_fft(x, 0.5, 1, endpoint=True)
