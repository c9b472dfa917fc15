"""The cross-spectrum handle on the MI355X: fourier_hip_csd_* through fourier_amd.CrossSpectrum and csd / coherence on torch tensors,
against tests/csd_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_csd_emu.py (it also covers the argument
checks of the C ABI and the allocation-free property after reserve); the chunk and row-group walks under a small scratch bound run on
the MI355X in tests/test_gpu_chunks.py, through the experiments library.

Inputs of every accuracy check: x white Gaussian, y = 0.6 roll(x, 5) + 0.8 independent white Gaussian (|Pxy| stays near 0.6 of
sqrt(Pxx Pyy), no bin near zero in norm), a window 0.5 + rand.  Tolerances, relative L2 over the whole output, with `base`
tests/test_gpu_stft.py's forward tolerance for the same inner plan and precision (2e-6 f32, 1e-13 f64, doubled on a Bluestein plan):
  CSD        4 x base.  d(conj X Y) <= |dX||Y| + |X||dY| is 2 x the STFT's relative error against |X||Y|; over the 0.6 above, 3.3 x.
  coherence  12 x base.  Twice the CSD's error plus the two power errors of 2 x base each: 10.7 x.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import csd_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
PAIRS = {128: 16, 256: 32, 512: 16, 1024: 8, 2048: 4}  # frame pairs per workgroup of the fused kernel at f32; half as many at f64


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


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (2e-13 if blu else 1e-13)


def tol(plan, real):
    return 4 * base(plan, real)


def tol_coherence(plan, real):
    return 12 * base(plan, real)


def dtypes(torch, real):
    return (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.CrossSpectrum(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode, 0)


def has_fused(real, n_fft):
    return n_fft in (128, 256, 512, 1024) or (n_fft == 2048 and real == "f32")


def pairs(real, n_fft):
    return PAIRS.get(n_fft, 32) // (1 if real == "f32" else 2)


def length_for(frames, n_fft, hop, pad_mode, extra):
    """a row length that gives `frames` frames, `extra` samples beyond the last frame's start rule"""
    return (frames - 1) * hop + extra + (n_fft if pad_mode == "none" else 0)


def pair(torch, g, shape, dt):
    x = torch.randn(*shape, dtype=dt, device="cuda", generator=g)
    y = 0.6 * torch.roll(x, 5, -1) + 0.8 * torch.randn(*shape, dtype=dt, device="cuda", generator=g)
    return x, y


def check(torch, fa, real, n_fft, hop, pad_mode="reflect", extra=3, batch=3, win_length=None, frames=None):
    """Frames per row = pairs per tile + 3 unless given: the last tile of every row is partly empty.  Both "fusion" values: the CSD with the fold
    and scale 0.37 into a buffer that starts on an odd element with a sentinel on both sides, and the coherence, against the truth; the
    two routes within tolerance of each other."""
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    rt, ct = dtypes(torch, real)
    frames = pairs(real, n_fft) + 3 if frames is None else frames
    length = length_for(frames, n_fft, hop, pad_mode, extra)
    g = torch.Generator(device="cuda").manual_seed(n_fft + hop + length)
    w = 0.5 + torch.rand(plan.win_length(), dtype=rt, device="cuda", generator=g)
    plan.set_window(w)
    x, y = pair(torch, g, (batch, length), rt)
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) == frames
    xh, yh, wh = x.cpu().numpy(), y.cpu().numpy(), w.cpu().numpy()
    want_p = truth.csd(xh, yh, n_fft, hop, plan.win_length(), wh, pad_mode, True, 0.37)
    want_c = truth.coherence(xh, yh, n_fft, hop, plan.win_length(), wh, pad_mode)
    count = batch * plan.bins()
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        route = "fused rows" if fusion == 1 and has_fused(real, n_fft) else "composed"
        d = plan.describe()
        assert d.startswith(f"csd {route}, coherence {route}: real "), d
        buf = torch.full((count + 3,), SENTINEL, dtype=ct, device="cuda")
        pxy = buf[1:1 + count].view(batch, plan.bins())
        assert plan.csd(x, y, True, 0.37, out=pxy) is pxy
        err = rel_l2(pxy.cpu().numpy(), want_p)
        print(f"csd {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} {route}: err {err:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real), (real, n_fft, hop, pad_mode, route, err)
        assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the CSD output was written"
        buf = torch.full((count + 3,), SENTINEL, dtype=rt, device="cuda")
        cxy = buf[1:1 + count].view(batch, plan.bins())
        assert plan.coherence(x, y, out=cxy) is cxy
        err = rel_l2(cxy.cpu().numpy(), want_c)
        print(f"coherence {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} {route}: err {err:.3g} tol {tol_coherence(plan, real):.3g}")
        assert err <= tol_coherence(plan, real), (real, n_fft, hop, pad_mode, route, err)
        assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the coherence output was written"
        got[fusion] = pxy.cpu().numpy(), cxy.cpu().numpy()
    assert rel_l2(got[1][0], got[0][0]) <= tol(plan, real)
    assert rel_l2(got[1][1], got[0][1]) <= tol_coherence(plan, real)
    return plan


def largest_fused(real):
    return 2048 if real == "f32" else 1024


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(torch, fa, real):
    for n in (128, 256, largest_fused(real)):
        check(torch, fa, real, n, n // 4, "reflect", extra=2)        # even rows and hop: pairs of reals
        check(torch, fa, real, n, n // 8 + 1, "reflect", extra=3)    # an odd hop: single reals
        check(torch, fa, real, n, n // 4, "constant", extra=5)       # zero padding, an odd length
        check(torch, fa, real, n, n // 4, "none", extra=6)           # no padding: every frame interior
        check(torch, fa, real, n, n // 4, "reflect", extra=2, win_length=n - 56)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_xcds(torch, fa, real):
    """6 tiles + 3 frames a row, batch 3: 3 * 7 = 21 workgroups, above 8 and no multiple of 8 -- the workgroup-to-block map
    (real_xcd_block) gives the first XCDs one block more than the rest, and the tile-to-row division (real_div) runs on blocks past the
    eighth.  check()'s assertions, with pairs of reals (even rows) and single reals (an odd length)."""
    for n in (256, largest_fused(real)):
        frames = 6 * pairs(real, n) + 3
        assert 3 * -(-frames // pairs(real, n)) == 21
        for pad_mode, extra in (("reflect", 2), ("none", 5)):
            plan = check(torch, fa, real, n, n // 4, pad_mode, extra=extra, frames=frames)
            plan.set_option("fusion", 1)
            assert plan.describe().startswith("csd fused rows, coherence fused rows"), plan.describe()


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_input_on_an_odd_element(torch, fa, real, fusion):
    """tests/test_gpu_stft.py's test of the same name for this handle.  An even hop, padding and row length: only the two base
    addresses decide whether the fused kernel loads pairs of reals, and it does only where both are aligned.  x aligned and y one
    element into its allocation, the reverse, both odd, and one odd buffer for both: against the truth, and bit-equal to what the
    same handle gives from aligned copies.  One buffer for both: conj(X) X is real, but a product contracted into a fused multiply-add
    may leave a rounding residue in Im, so the CSD is held to the truth's csd(x, x) and the coherence to 1."""
    rt, _ = dtypes(torch, real)
    for n in (256, largest_fused(real)):
        hop, batch = n // 4, 3
        frames = pairs(real, n) + 3
        length = length_for(frames, n, hop, "reflect", 2)
        assert hop % 2 == 0 and length % 2 == 0
        g = torch.Generator(device="cuda").manual_seed(n + fusion)
        xa, ya = pair(torch, g, (batch, length), rt)
        holders = [torch.zeros(batch * length + 2, dtype=rt, device="cuda") for _ in range(2)]
        xo, yo = (h[1:-1].view(batch, length) for h in holders)
        xo.copy_(xa)
        yo.copy_(ya)
        before = [h.clone() for h in holders]
        two = 2 * xa.element_size()
        assert xo.data_ptr() % two != 0 and yo.data_ptr() % two != 0 and xa.data_ptr() % two == 0 and ya.data_ptr() % two == 0
        plan = make(fa, real, n, hop)
        w = 0.5 + torch.rand(n, dtype=rt, device="cuda", generator=g)
        plan.set_window(w)
        plan.set_option("fusion", fusion)
        assert plan.describe().startswith("csd fused rows" if fusion else "csd composed"), plan.describe()
        assert plan.frames(length) == frames
        xh, yh, wh = xa.cpu().numpy(), ya.cpu().numpy(), w.cpu().numpy()
        want_p = truth.csd(xh, yh, n, hop, n, wh, "reflect", True, 0.37)
        want_c = truth.coherence(xh, yh, n, hop, n, wh, "reflect")
        aligned_p, aligned_c = plan.csd(xa, ya, True, 0.37), plan.coherence(xa, ya)
        for name, x, y in (("x aligned, y odd", xa, yo), ("x odd, y aligned", xo, ya), ("both odd", xo, yo)):
            got_p, got_c = plan.csd(x, y, True, 0.37), plan.coherence(x, y)
            ep, ec = rel_l2(got_p.cpu().numpy(), want_p), rel_l2(got_c.cpu().numpy(), want_c)
            print(f"csd odd input {real} n_fft={n} fusion={fusion} {name}: csd err {ep:.3g} tol {tol(plan, real):.3g} "
                  f"coherence err {ec:.3g} tol {tol_coherence(plan, real):.3g}")
            assert ep <= tol(plan, real) and ec <= tol_coherence(plan, real), (real, n, fusion, name, ep, ec)
            assert torch.equal(torch.view_as_real(got_p), torch.view_as_real(aligned_p)) and torch.equal(got_c, aligned_c), (real, n, fusion, name)
        got_p, got_c = plan.csd(xo, xo, True, 0.37), plan.coherence(xo, xo)
        ep = rel_l2(got_p.cpu().numpy(), truth.csd(xh, xh, n, hop, n, wh, "reflect", True, 0.37))
        ec = float(np.max(np.abs(got_c.cpu().numpy().astype(np.float64) - 1)))
        print(f"csd odd input {real} n_fft={n} fusion={fusion} y is x: csd err {ep:.3g} tol {tol(plan, real):.3g} "
              f"max |coherence - 1| {ec:.3g} tol {tol_coherence(plan, real):.3g}")
        assert ep <= tol(plan, real) and ec <= tol_coherence(plan, real), (real, n, fusion, ep, ec)
        assert torch.equal(torch.view_as_real(got_p), torch.view_as_real(plan.csd(xa, xa, True, 0.37))), (real, n, fusion, "y is x")
        assert torch.equal(got_c, plan.coherence(xa, xa)), (real, n, fusion, "y is x")
        assert all(torch.equal(h, b) for h, b in zip(holders, before)), "a call modified an input"


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(torch, fa, real):
    for n, hop, pad_mode in ((400, 100, "reflect"), (400, 37, "none"), (255, 63, "reflect"), (255, 64, "constant")):
        plan = check(torch, fa, real, n, hop, pad_mode)  # 35 frames a row: two slots of partials, the last partly used
        assert plan.describe().startswith("csd composed, coherence composed"), plan.describe()


@pytest.mark.parametrize("n_fft", [128, 256, 512, 1024, 2048])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_results_are_repeatable(torch, fa, real, n_fft):
    """Every fused instantiation, both results, ten times into fresh outputs: bit-equal to the first (a race on the kernel's LDS
    buffers, or a sum whose order moves, shows as a difference between runs).  Where the precision has no fused kernel of the length
    the composed route runs."""
    n, hop = n_fft, n_fft // 4
    g = torch.Generator(device="cuda").manual_seed(n)
    rt, _ = dtypes(torch, real)
    frames, batch = 2 * pairs(real, n) + 3, 3
    length = length_for(frames, n, hop, "reflect", 3)
    x, y = pair(torch, g, (batch, length), rt)
    plan = make(fa, real, n, hop)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("csd fused rows" if has_fused(real, n) else "csd composed"), plan.describe()
    runs = [(plan.csd(x, y), plan.coherence(x, y)) for _ in range(10)]
    torch.cuda.synchronize()
    err = rel_l2(runs[0][0].cpu().numpy(), truth.csd(x.cpu().numpy(), y.cpu().numpy(), n, hop, pad_mode="reflect"))
    print(f"csd repeat {real} n_fft={n}: err {err:.3g} tol {tol(plan, real):.3g}")
    assert err <= tol(plan, real), (real, n, err)
    err = rel_l2(runs[0][1].cpu().numpy(), truth.coherence(x.cpu().numpy(), y.cpu().numpy(), n, hop, pad_mode="reflect"))
    print(f"coherence repeat {real} n_fft={n}: err {err:.3g} tol {tol_coherence(plan, real):.3g}")
    assert err <= tol_coherence(plan, real), (real, n, err)
    for i, run in enumerate(runs[1:]):
        assert all(torch.equal(a, b) for a, b in zip(run, runs[0])), (real, n, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """csd and coherence captured on a side stream as the first calls of a handle that reserved (they must not allocate), one linear
    graph, replayed twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, hop, length, batch = 256, 64, 5 * 256, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [pair(torch, g, (batch, length), torch.float32) for _ in range(3)]
    w = 0.5 + torch.rand(n, dtype=torch.float32, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = make(fa, "f32", n, hop)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.csd(*xs[0])
        other.coherence(*xs[0])
    side.synchronize()
    plan = make(fa, "f32", n, hop)
    plan.set_option("fusion", fusion)
    plan.set_window(w)
    assert plan.describe().startswith("csd fused rows" if fusion else "csd composed"), plan.describe()
    plan.reserve(length, batch)
    torch.cuda.synchronize()
    dx, dy = xs[0][0].clone(), xs[0][1].clone()
    P = torch.empty(batch, plan.bins(), dtype=torch.complex64, device="cuda")
    C = torch.empty(batch, plan.bins(), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.csd(dx, dy, out=P)  # the first calls on this plan: captured
        plan.coherence(dx, dy, out=C)
    wh = w.cpu().numpy()
    for x, y in xs[1:]:
        dx.copy_(x)
        dy.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        eP, eC = plan.csd(x, y), plan.coherence(x, y)
        torch.cuda.synchronize()
        assert torch.equal(P, eP) and torch.equal(C, eC), fusion
        xh, yh = x.cpu().numpy(), y.cpu().numpy()
        assert rel_l2(P.cpu().numpy(), truth.csd(xh, yh, n, hop, n, wh, "reflect")) <= tol(plan, "f32")
        assert rel_l2(C.cpu().numpy(), truth.coherence(xh, yh, n, hop, n, wh, "reflect")) <= tol_coherence(plan, "f32")


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    for real in ("f32", "f64"):
        rt, ct = dtypes(torch, real)
        x, y = pair(torch, g, (2, 3, 2000), rt)
        xh, yh = x.reshape(6, 2000).cpu().numpy(), y.reshape(6, 2000).cpu().numpy()
        # scipy's definition without detrending, against the truth: both scalings, one-sided and not
        for nperseg, noverlap, scaling, onesided, fs in ((256, None, "density", True, 48.0), (255, 100, "spectrum", True, 1.0),
                                                         (400, 0, "density", False, 2.0)):
            nov = nperseg // 2 if noverlap is None else noverlap
            plan = fa.CrossSpectrum(nperseg, real, nperseg - nov, center=False, device=0)
            f, P = fa.csd(x, y, fs, None, nperseg, noverlap, scaling, onesided)
            wh = torch.hann_window(nperseg, periodic=True, dtype=torch.float64).to(rt).numpy()
            want = truth.csd(xh, yh, nperseg, nperseg - nov, nperseg, wh, "none", onesided, truth.welch_scale(wh, fs, scaling))
            assert P.shape == (2, 3, nperseg // 2 + 1) and P.dtype == ct and f.shape == (nperseg // 2 + 1,) and f.dtype == rt
            assert np.allclose(f.cpu().numpy(), np.arange(nperseg // 2 + 1) * fs / nperseg, rtol=1e-6)
            err = rel_l2(P.reshape(6, -1).cpu().numpy(), want)
            print(f"torch csd {real} nperseg={nperseg} {scaling}: err {err:.3g} tol {tol(plan, real):.3g}")
            assert err <= tol(plan, real), (real, nperseg, err)
            f, C = fa.coherence(x, y, fs, None, nperseg, noverlap)
            assert C.shape == (2, 3, nperseg // 2 + 1) and C.dtype == rt and f.shape == (nperseg // 2 + 1,)
            err = rel_l2(C.reshape(6, -1).cpu().numpy(), truth.coherence(xh, yh, nperseg, nperseg - nov, nperseg, wh, "none"))
            print(f"torch coherence {real} nperseg={nperseg}: err {err:.3g} tol {tol_coherence(plan, real):.3g}")
            assert err <= tol_coherence(plan, real), (real, nperseg, err)
        wt = 0.5 + torch.rand(256, dtype=rt, device="cuda", generator=g)
        f, P = fa.csd(x, y, 8.0, wt, 256, 192, "spectrum")
        want = truth.csd(xh, yh, 256, 64, 256, wt.cpu().numpy(), "none", True, truth.welch_scale(wt.cpu().numpy(), 8.0, "spectrum"))
        assert rel_l2(P.reshape(6, -1).cpu().numpy(), want) <= 4 * (2e-6 if real == "f32" else 1e-13)
        # out= on the handle, folded leading dimensions.  The scale here is numpy's sum of the window and the module function's is
        # torch's, which may differ in the last place at f64: out= is bit-equal to the same handle's own return, and held to the truth
        # by the bound P is held to
        plan = fa.CrossSpectrum(256, real, 64, center=False, device=0)
        plan.set_window(wt)
        scale = float(truth.welch_scale(wt.cpu().numpy(), 8.0, "spectrum"))
        out = torch.empty(2, 3, 129, dtype=ct, device="cuda")
        assert plan.csd(x, y, True, scale, out=out) is out and torch.equal(out, plan.csd(x, y, True, scale))
        assert rel_l2(out.reshape(6, -1).cpu().numpy(), want) <= 4 * (2e-6 if real == "f32" else 1e-13)
        outc = torch.empty(2, 3, 129, dtype=rt, device="cuda")
        assert plan.coherence(x, y, out=outc) is outc and torch.equal(outc, fa.coherence(x, y, 8.0, wt, 256, 192)[1])
        assert plan.csd(x[0, 0], y[0, 0]).shape == (129,)
        with pytest.raises(TypeError):
            plan.csd(x, y, out=torch.empty(2, 3, 129, dtype=ct))               # not on the device
        with pytest.raises(TypeError):
            plan.csd(x, y, out=torch.empty(2, 3, 129, dtype=rt, device="cuda"))  # not complex
        with pytest.raises(TypeError):
            plan.coherence(x, y, out=torch.empty(6, 129, dtype=rt, device="cuda"))  # not the folded shape
        with pytest.raises(ValueError):
            plan.csd(x, y[:1])
        with pytest.raises(TypeError):
            plan.csd(x, y.to(torch.float64 if real == "f32" else torch.float32))
    x, y = pair(torch, g, (4, 1000), torch.float32)
    for fn in (fa.csd, fa.coherence):
        with pytest.raises(TypeError):
            fn(x.cpu(), y)
        with pytest.raises(TypeError):
            fn(x, y.cpu())
        with pytest.raises(TypeError):
            fn(x, y.double())                    # mismatched dtypes
        with pytest.raises(TypeError):
            fn(x.to(torch.complex64), y)
        with pytest.raises(ValueError):
            fn(x, y[:, :999])                    # mismatched shapes
        with pytest.raises(ValueError):
            fn(x, y[:2])
        with pytest.raises(ValueError):
            fn(x, y, nperseg=2000)               # longer than the rows
        with pytest.raises(ValueError):
            fn(x, y, nperseg=256, noverlap=256)
        with pytest.raises(ValueError):
            fn(x, y, fs=0.0)
        with pytest.raises(ValueError):
            fn(x, y, window=torch.ones(100, device="cuda"))
        with pytest.raises(TypeError):
            fn(x, y, window=torch.ones(256, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fa.csd(x, y, scaling="psd")
