"""Linear convolution with a prepared filter bank on the MI355X: fourier_hip_lconv_* through the C ABI (LinearConv.apply_ptr /
set_filters_ptr), LinearConv.apply and fftconvolve on torch tensors, against numpy.convolve / numpy.correlate in f64 on the same
(rounded) inputs, sliced to the mode.  The CPU twin is tests/test_lconv_emu.py (argument checks, the route rule, the chunk walk, the
allocation-free property after reserve).

Tolerance, relative L2 over the whole output: tests/test_gpu_conv.py's, three transforms' worth: 6e-6 (f32) and 3e-13 (f64) on the
overlap-save route and on the padded route over a plan that is not a Bluestein one, that file's tol() otherwise.  The real pairing
passes the same arithmetic as the complex kernel and has no tolerance of its own.
"""
import numpy as np
import pytest

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
    return 3 * ((4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13))


def dtype_of(torch, real, real_data):
    if real_data:
        return torch.float32 if real == "f32" else torch.float64
    return torch.complex64 if real == "f32" else torch.complex128


def geometry(lx, k, mode):
    return {"full": (0, lx + k - 1), "same": ((k - 1) // 2, lx), "valid": (k - 1, lx - k + 1)}[mode]


def want(x, h, mode, correlate=False):
    """numpy in f64, row b with filter b mod F, sliced by the table of include/fourier.h (long taps: the same sums through an FFT in f64)"""
    h = np.atleast_2d(h)
    lx, k = x.shape[-1], h.shape[-1]
    wide = np.complex128 if np.iscomplexobj(x) else np.float64
    off, lout = geometry(lx, k, mode)
    rows = []
    for b in range(x.shape[0]):
        hb = h[b % h.shape[0]].astype(wide)
        if correlate:
            hb = np.conj(hb[::-1])
        if k > 1024:  # the same sums through numpy's FFT in f64: its own error is some 1e-16 per value, far below every tolerance here
            m = lx + k - 1
            full = np.fft.ifft(np.fft.fft(x[b].astype(np.complex128), m) * np.fft.fft(hb.astype(np.complex128), m))
            full = full if wide is np.complex128 else full.real
        else:
            full = np.convolve(x[b].astype(wide), hb)
        rows.append(full[off:off + lout])
    return np.array(rows)


def run(torch, plan, x, h, correlate=False):
    """set the filters, apply into a buffer with a guard row in front and behind, check the guards and the inputs"""
    stream = torch.cuda.current_stream().cuda_stream
    h2 = h.reshape(-1, h.shape[-1])
    xh, hh = x.cpu().numpy(), h2.cpu().numpy()
    plan.set_filters_ptr(h2.data_ptr(), h2.shape[0], correlate, stream)
    batch, lout = x.numel() // x.shape[-1], plan.out_length()
    buf = torch.full((batch + 2, lout), SENTINEL, dtype=x.dtype, device="cuda")
    plan.apply_ptr(x.data_ptr(), buf[1:].data_ptr(), batch, stream)
    out = buf.cpu().numpy()
    assert np.all(out[0] == SENTINEL) and np.all(out[-1] == SENTINEL), "a guard row was written"
    assert np.array_equal(x.cpu().numpy(), xh) and np.array_equal(h2.cpu().numpy(), hh), "apply modified its input or the taps"
    return out[1:-1]


def check(torch, fa, lx, k, real, real_data, mode, batch=2, F=1, correlate=False, block=0, overlap_save=1, describe=None, seed=0):
    dt = dtype_of(torch, real, real_data)
    plan = fa.LinearConv(lx, k, real, mode, real_data, 0)
    if block:
        plan.set_option("block", block)
    if not overlap_save:
        plan.set_option("overlap_save", 0)
    if describe is not None:
        assert plan.describe().startswith(describe), (lx, k, real, real_data, plan.describe())
    g = torch.Generator(device="cuda").manual_seed(seed + lx + k)
    x = torch.randn(batch, lx, dtype=dt, device="cuda", generator=g)
    h = torch.randn(F, k, dtype=dt, device="cuda", generator=g)
    got = run(torch, plan, x, h, correlate)
    w = want(x.cpu().numpy(), h.cpu().numpy(), mode, correlate)
    err = rel_l2(got, w)
    print(f"lconv {real} {'real' if real_data else 'complex'} Lx={lx} K={k} {mode} batch={batch} F={F}: rel_l2 {err:.3e}  [{plan.describe()}]")
    assert got.shape == w.shape and err <= tol(plan, real), (lx, k, real, real_data, mode, err, plan.describe())
    return plan


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_block_shape(torch, fa, real, real_data):
    for v in range(11, 16 if real == "f32" else 15):
        n = 1 << v
        for mode in ("full", "same"):
            check(torch, fa, 2 * n + 37, n // 8 + 1, real, real_data, mode, batch=3, block=v, describe=f"lconv overlap-save: block {n} ")


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_the_block_rule(torch, fa, real, real_data):
    # (f32 takes the block of 8 (K - 1) up to 2^13, f64 the block of 4 (K - 1): include/fourier.h)
    for k, n in ((5, 2048), (129, 2048), (1025, 8192 if real == "f32" else 4096), (4097, 16384)):
        check(torch, fa, 70001, k, real, real_data, "valid", describe=f"lconv overlap-save: block {n} ")


# tests/test_lconv_emu.py's shapes at block 2^11: three blocks with a partial last one; odd rows and SAME offset 15; one block; K > Lx
# (FULL only); K = 1; five blocks
SHAPES = [(5000, 33), (4999, 32), (1900, 7), (40, 64), (3000, 1), (9000, 100)]


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_edges_through_the_c_abi(torch, fa, real, real_data):
    for lx, k in SHAPES:
        for mode in ("full", "same", "valid"):
            if k > lx and mode != "full":
                continue
            check(torch, fa, lx, k, real, real_data, mode, batch=7, F=3, correlate=(mode == "same"),
                  describe="lconv overlap-save: block 2048 ")


def test_tensor_entry_points(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(11)
    for dt, real, real_data in ((torch.complex64, "f32", False), (torch.float64, "f64", True), (torch.float32, "f32", True)):
        for lx, k in SHAPES:
            for mode in ("full", "same", "valid"):
                if k > lx and mode != "full":
                    continue
                x = torch.randn(2, 3, lx, dtype=dt, device="cuda", generator=g)
                h = torch.randn(3, k, dtype=dt, device="cuda", generator=g)
                xh, hh = x.cpu().numpy().reshape(6, lx), h.cpu().numpy()
                lout = geometry(lx, k, mode)[1]
                w = want(xh, hh, mode).reshape(2, 3, lout)
                t = 6e-6 if real == "f32" else 3e-13
                y = fa.fftconvolve(x, h, mode)
                assert tuple(y.shape) == (2, 3, lout) and rel_l2(y.cpu().numpy(), w) <= t, (dt, lx, k, mode)
                out = torch.empty(2, 3, lout, dtype=dt, device="cuda")
                assert fa.fftconvolve(x, h, mode, out=out) is out and rel_l2(out.cpu().numpy(), w) <= t
                wc = want(xh, hh[1], mode, True).reshape(2, 3, lout)
                yc = fa.fftconvolve(x, h[1].contiguous(), mode, correlate=True)  # the cached handle, a new bank of one filter
                assert rel_l2(yc.cpu().numpy(), wc) <= t, (dt, lx, k, mode, "correlate")
                wn = np.correlate(xh[0].astype(w.dtype), hh[1].astype(w.dtype), mode) if k <= lx else None  # numpy's own, one row
                if wn is not None:
                    assert rel_l2(yc.cpu().numpy()[0, 0], wn) <= t
        plan = fa.LinearConv(1900, 7, real, "same", real_data)
        x = torch.randn(4, 1900, dtype=dt, device="cuda", generator=g)
        with pytest.raises(TypeError):
            plan.set_filters(torch.ones(7, dtype=dt))
        with pytest.raises(ValueError):
            plan.set_filters(torch.ones(8, dtype=dt, device="cuda"))
        plan.set_filters(torch.ones(7, dtype=dt, device="cuda"))
        with pytest.raises(TypeError):
            plan.apply(x.cpu())
        with pytest.raises(TypeError):
            plan.apply(x.transpose(0, 1))
        with pytest.raises(ValueError):
            plan.apply(x[..., :1899].contiguous())
        with pytest.raises(TypeError):
            plan.apply(x, out=torch.empty(4, 1901, dtype=dt, device="cuda"))
        with pytest.raises(fa.FourierError):
            plan.apply(x, out=x)  # in place is not allowed
        with pytest.raises(TypeError):
            fa.fftconvolve(x.cpu(), torch.ones(7, dtype=dt, device="cuda"))
        with pytest.raises(ValueError):
            fa.fftconvolve(x, torch.ones(7, dtype=dt, device="cuda"), mode="causal")


def test_offsets_past_2p25_bytes_and_rejected_accesses_at_both_row_ends(torch, fa):
    """A row just under the 2^31-byte cap is out of reach of a test of seconds; this one has byte offsets past 2^25 and, with an odd
    length and two rows, rejected accesses in front of the first row's start (next to the guard row) and behind every row's end."""
    lx, k = (1 << 22) + 3, 129
    plan = fa.LinearConv(lx, k, "f32", "full", False, 0)
    assert plan.describe().startswith("lconv overlap-save: block 2048 ")
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(2, lx, dtype=torch.complex64, device="cuda", generator=g)
    h = torch.randn(1, k, dtype=torch.complex64, device="cuda", generator=g)
    got = run(torch, plan, x, h)
    xh, hh = x.cpu().numpy().astype(np.complex128), h.cpu().numpy().astype(np.complex128)[0]
    lout = lx + k - 1
    for b in range(2):
        for lo in (0, lout // 2 - 2048, lout - 4096):
            # outputs lo ... lo + 4095 of the full convolution need inputs lo - (K - 1) ... lo + 4095
            a = max(0, lo - (k - 1))
            seg = np.convolve(xh[b, a:min(lx, lo + 4096)], hh)[lo - a:lo - a + 4096]
            err = rel_l2(got[b, lo:lo + 4096], seg)
            assert err <= 6e-6, (b, lo, err)


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
def test_padded_route_with_long_taps(torch, fa, real_data):
    for real in ("f32", "f64"):
        check(torch, fa, 30000, 20000, real, real_data, "full", batch=3, F=2, describe="lconv padded: M=65536, conv ")
        check(torch, fa, 30000, 20000, real, real_data, "valid", batch=3, F=2, correlate=True, describe="lconv padded: M=65536, conv ")
        check(torch, fa, 1, 1, real, real_data, "full", batch=5, F=2, overlap_save=0, describe="lconv padded: M=1, conv ")


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_the_two_routes_agree(torch, fa, real, real_data):
    lx, k = 10000, 200
    for mode in ("full", "same", "valid"):
        a = check(torch, fa, lx, k, real, real_data, mode, batch=5, F=2, describe="lconv overlap-save: ")
        b = check(torch, fa, lx, k, real, real_data, mode, batch=5, F=2, overlap_save=0, describe="lconv padded: ")
        dt = dtype_of(torch, real, real_data)
        g = torch.Generator(device="cuda").manual_seed(17)
        x = torch.randn(5, lx, dtype=dt, device="cuda", generator=g)
        h = torch.randn(2, k, dtype=dt, device="cuda", generator=g)
        ya, yb = run(torch, a, x, h), run(torch, b, x, h)
        assert rel_l2(ya, yb) <= tol(a, real) + tol(b, real), (real, real_data, mode)


@pytest.mark.parametrize("overlap_save", [1, 0], ids=["overlap-save", "padded"])
def test_graph_replay_of_apply_after_reserve(torch, fa, overlap_save):
    lx, k, batch = 50000, 65, 8
    g = torch.Generator(device="cuda").manual_seed(12)
    x0 = torch.randn(batch, lx, dtype=torch.complex64, device="cuda", generator=g)
    x1 = torch.randn(batch, lx, dtype=torch.complex64, device="cuda", generator=g)
    h = torch.randn(3, k, dtype=torch.complex64, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = fa.LinearConv(lx, k, "f32", "same")  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("overlap_save", overlap_save)
    with torch.cuda.stream(side):
        other.set_filters(h)
        other.apply(x0)
    side.synchronize()
    plan = fa.LinearConv(lx, k, "f32", "same")
    plan.set_option("overlap_save", overlap_save)
    assert plan.describe().startswith("lconv overlap-save: " if overlap_save else "lconv padded: ")
    plan.set_filters(h)
    plan.reserve(batch)
    torch.cuda.synchronize()
    d, o = x0.clone(), torch.empty_like(x0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.apply(d, out=o)  # the first apply on this plan: captured, must not allocate
    d.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    eager = plan.apply(x1)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), eager.cpu().numpy())
    assert rel_l2(o.cpu().numpy(), want(x1.cpu().numpy(), h.cpu().numpy(), "same")) <= tol(plan, "f32")


def existing_outputs(torch, fa):
    """Fft and FftConv outputs at 2^12 and 2^20 on seeded inputs (the same in every process)"""
    g = torch.Generator(device="cuda").manual_seed(19)
    res = []
    for n in (1 << 12, 1 << 20):
        x = torch.randn(3, n, dtype=torch.complex64, device="cuda", generator=g)
        h = torch.randn(2, 33, dtype=torch.complex64, device="cuda", generator=g)
        y = torch.empty_like(x)
        fa.Fft(n, "f32", 0).transform_batch_ptr(x.data_ptr(), y.data_ptr(), 3, fa.Transform.Fft, torch.cuda.current_stream().cuda_stream)
        conv = fa.FftConv(n, "f32", False, 0)
        conv.set_filters(h)
        res += [y.cpu().numpy(), conv.apply(x).cpu().numpy()]
    return res


def test_existing_handles_are_untouched(torch, fa, tmp_path):
    """The baseline comes from a fresh process that never creates an lconv handle (this one may have used many by now); this process
    then creates and uses lconv handles on both routes and both kinds of data and must reproduce the baseline bit for bit."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "baseline.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy, torch, fourier_amd, test_gpu_lconv\n"
            "numpy.savez(%r, *test_gpu_lconv.existing_outputs(torch, fourier_amd))\n" % (here, os.path.dirname(here), path))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as z:
        before = [z[f"arr_{i}"] for i in range(4)]
    for real_data in (False, True):
        for overlap_save in (1, 0):
            check(torch, fa, 9000, 100, "f32", real_data, "same", overlap_save=overlap_save)
    after = existing_outputs(torch, fa)
    assert len(after) == 4 and all(np.array_equal(a, b) for a, b in zip(before, after))
