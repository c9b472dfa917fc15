"""The spectrogram handle on the MI355X: fourier_hip_spectrogram_* through fourier_amd.Spectrogram and spectrogram / welch on torch
tensors, against tests/spectrogram_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_spectrogram_emu.py (it also
covers the argument checks and the allocation-free property after reserve); the chunk and row-group walks under a small scratch bound
run on the MI355X in tests/test_gpu_chunks.py, through the experiments library.

Tolerance, relative L2 over the whole output on white Gaussian input (no bin near zero in norm): twice the forward tolerance
tests/test_gpu_stft.py's tol() gives the same inner plan and precision.  d|X|^2 = 2 Re(conj X dX) makes the relative error of a power
about 1.4 x the STFT's; a square root or a mean over frames does not raise it.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import spectrogram_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
TILE = {128: 32, 256: 64, 512: 32, 1024: 16, 2048: 8}  # frames per workgroup of the fused kernel at f32; half as many at f64


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
    return 2 * 2 * base  # twice tests/test_gpu_stft.py's forward tolerance


def rdtype(torch, real):
    return torch.float32 if real == "f32" else torch.float64


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.Spectrogram(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode, 0)


def has_fused(real, n_fft):
    return n_fft in (128, 256, 512, 1024) or (n_fft == 2048 and real == "f32")


def cols(real, n_fft):
    return TILE.get(n_fft, 32) // (1 if real == "f32" else 2)


def length_for(frames, n_fft, hop, pad_mode, extra):
    """a row length that gives `frames` frames, `extra` samples beyond the last frame's start rule"""
    return (frames - 1) * hop + extra + (n_fft if pad_mode == "none" else 0)


def check(torch, fa, real, n_fft, hop, pad_mode="reflect", extra=3, batch=3, win_length=None, frames=None):
    """Frames per row = tile + 3 unless given: the last tile of every row is partly empty (Welch) and tiles straddle rows (spectrogram).  Both
    "fusion" values, magnitude and power into a buffer that starts on an odd element with a sentinel on both sides, Welch with the
    fold against the truth and without it against the mean of the handle's own power spectrogram."""
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    dt = rdtype(torch, real)
    frames = cols(real, n_fft) + 3 if frames is None else frames
    length = length_for(frames, n_fft, hop, pad_mode, extra)
    g = torch.Generator(device="cuda").manual_seed(n_fft + hop + length)
    w = 0.5 + torch.rand(plan.win_length(), dtype=dt, device="cuda", generator=g)
    plan.set_window(w)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) == frames
    xh, wh = x.cpu().numpy(), w.cpu().numpy()
    count = batch * frames * plan.bins()
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        route = "fused rows" if fusion == 1 and has_fused(real, n_fft) else "composed"
        d = plan.describe()
        assert d.startswith(f"spectrogram {route}, welch {route}: real "), d
        for power in (1, 2):
            normalized = power == 1
            buf = torch.full((count + 3,), SENTINEL, dtype=dt, device="cuda")
            out = buf[1:1 + count].view(batch, frames, plan.bins())
            assert out.data_ptr() % (2 * out.element_size()) != 0
            assert plan.forward(x, power, normalized, out=out) is out
            want = truth.spectrogram(xh, n_fft, hop, plan.win_length(), wh, pad_mode, power, normalized)
            err = rel_l2(out.cpu().numpy(), want)
            print(f"spectrogram {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} power={power} {route}: err {err:.3g} "
                  f"tol {tol(plan, real):.3g}")
            assert err <= tol(plan, real), (real, n_fft, hop, pad_mode, power, route, err)
            assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the output was written"
            got[fusion, power] = out.clone()
        buf = torch.full((batch * plan.bins() + 3,), SENTINEL, dtype=dt, device="cuda")
        pxx = buf[1:1 + batch * plan.bins()].view(batch, plan.bins())
        assert plan.welch(x, True, 0.37, out=pxx) is pxx
        err = rel_l2(pxx.cpu().numpy(), truth.welch(xh, n_fft, hop, plan.win_length(), wh, pad_mode, True, 0.37))
        print(f"welch {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} {route}: err {err:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real), (real, n_fft, hop, pad_mode, route, err)
        assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the Welch output was written"
        mean = got[fusion, 2].cpu().numpy().astype(np.float64).mean(axis=1)
        err = rel_l2(plan.welch(x, False, 1.0).cpu().numpy(), mean)
        print(f"welch vs mean of the power spectrogram {real} n_fft={n_fft} {route}: err {err:.3g}")
        assert err <= tol(plan, real), (real, n_fft, hop, pad_mode, route, err)
    for power in (1, 2):
        assert rel_l2(got[1, power].cpu().numpy(), got[0, power].cpu().numpy()) <= tol(plan, real)
    return plan


def largest_fused(real):
    return 2048 if real == "f32" else 1024


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(torch, fa, real):
    for n in (256, largest_fused(real)):
        check(torch, fa, real, n, n // 4, "reflect", extra=2)        # even rows and hop: pairs of reals
        check(torch, fa, real, n, n // 8 + 1, "reflect", extra=3)    # an odd hop, an odd length: single reals
        check(torch, fa, real, n, n // 4, "constant", extra=5)       # zero padding, an odd length
        check(torch, fa, real, n, n // 4, "none", extra=6)           # no padding: every frame interior
    check(torch, fa, real, 256, 64, "reflect", extra=2, win_length=200)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_xcds(torch, fa, real):
    """6 tiles + 3 frames a row, batch 3: the spectrogram launches ceil(3 * (6 tile + 3) / tile) = 19 workgroups (20 at a tile of 8
    frames, n_fft = 2048) and Welch 3 * 7 = 21, all above 8 and no multiple of 8 -- the workgroup-to-block map (real_xcd_block) gives the first XCDs one block more than the rest,
    and the tile-to-row division (real_div) runs on blocks past the eighth.  check()'s assertions, with pairs of reals (even rows) and
    single reals (an odd length)."""
    for n in (256, largest_fused(real)):
        frames = 6 * cols(real, n) + 3
        forward_wgs, welch_wgs = -(-3 * frames // cols(real, n)), 3 * -(-frames // cols(real, n))
        assert forward_wgs == (20 if cols(real, n) == 8 else 19) and welch_wgs == 21
        assert all(wgs > 8 and wgs % 8 != 0 for wgs in (forward_wgs, welch_wgs))
        for pad_mode, extra in (("reflect", 2), ("none", 5)):
            plan = check(torch, fa, real, n, n // 4, pad_mode, extra=extra, frames=frames)
            plan.set_option("fusion", 1)
            assert plan.describe().startswith("spectrogram fused rows, welch fused rows"), plan.describe()


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_input_on_an_odd_element(torch, fa, real, fusion):
    """tests/test_gpu_stft.py's test of the same name for this handle.  An even hop, padding and row length: only the base address
    decides whether the fused kernels load pairs of reals.  Rows that start one element into their allocation against the truth, and
    bit-equal to what the same handle gives from an aligned copy of them; the input buffer itself untouched."""
    dt = rdtype(torch, real)
    for n in (256, largest_fused(real)):
        hop, batch = n // 4, 3
        frames = cols(real, n) + 3
        length = length_for(frames, n, hop, "reflect", 2)
        assert hop % 2 == 0 and length % 2 == 0
        g = torch.Generator(device="cuda").manual_seed(n + fusion)
        holder = torch.randn(batch * length + 2, dtype=dt, device="cuda", generator=g)
        before = holder.clone()
        x = holder[1:-1].view(batch, length)
        xa = x.clone()
        assert x.data_ptr() % (2 * x.element_size()) != 0 and xa.data_ptr() % (2 * x.element_size()) == 0
        plan = make(fa, real, n, hop)
        w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
        plan.set_window(w)
        plan.set_option("fusion", fusion)
        assert plan.describe().startswith("spectrogram fused rows" if fusion else "spectrogram composed"), plan.describe()
        assert plan.frames(length) == frames
        xh, wh = xa.cpu().numpy(), w.cpu().numpy()
        for power, normalized in ((2, False), (1, True)):
            got, aligned = plan.forward(x, power, normalized), plan.forward(xa, power, normalized)
            err = rel_l2(got.cpu().numpy(), truth.spectrogram(xh, n, hop, n, wh, "reflect", power, normalized))
            print(f"spectrogram odd input {real} n_fft={n} fusion={fusion} power={power}: err {err:.3g} tol {tol(plan, real):.3g}")
            assert err <= tol(plan, real), (real, n, fusion, power, err)
            assert torch.equal(got, aligned), (real, n, fusion, power)
        got, aligned = plan.welch(x, True, 0.37), plan.welch(xa, True, 0.37)
        err = rel_l2(got.cpu().numpy(), truth.welch(xh, n, hop, n, wh, "reflect", True, 0.37))
        print(f"welch odd input {real} n_fft={n} fusion={fusion}: err {err:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real), (real, n, fusion, err)
        assert torch.equal(got, aligned), (real, n, fusion, "welch")
        assert torch.equal(holder, before), "a call modified its input"


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(torch, fa, real):
    for n, hop, pad_mode in ((400, 100, "reflect"), (400, 37, "none"), (255, 63, "reflect"), (255, 64, "constant")):
        plan = check(torch, fa, real, n, hop, pad_mode)
        assert plan.describe().startswith("spectrogram composed, welch composed"), plan.describe()


@pytest.mark.parametrize("n_fft", [128, 256, 512, 1024, 2048])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_results_are_repeatable(torch, fa, real, n_fft):
    """Every fused instantiation, all three epilogues, ten times into fresh outputs: bit-equal to the first (a race on the kernel's LDS
    buffers, or a sum whose order moves, shows as a difference between runs).  Where the precision has no fused kernel of the length
    the composed route runs."""
    n, hop = n_fft, n_fft // 4
    g = torch.Generator(device="cuda").manual_seed(n)
    dt = rdtype(torch, real)
    frames, batch = cols(real, n) + 3, 3
    length = length_for(frames, n, hop, "reflect", 3)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    plan = make(fa, real, n, hop)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("spectrogram fused rows" if has_fused(real, n) else "spectrogram composed"), plan.describe()
    runs = [(plan.forward(x, 2), plan.forward(x, 1), plan.welch(x)) for _ in range(10)]
    torch.cuda.synchronize()
    err = rel_l2(runs[0][2].cpu().numpy(), truth.welch(x.cpu().numpy(), n, hop, pad_mode="reflect"))
    print(f"welch repeat {real} n_fft={n}: err {err:.3g} tol {tol(plan, real):.3g}")
    assert err <= tol(plan, real), (real, n, err)
    for i, run in enumerate(runs[1:]):
        assert all(torch.equal(a, b) for a, b in zip(run, runs[0])), (real, n, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """forward and welch captured on a side stream as the first calls of a handle that reserved (they must not allocate), one linear
    graph, replayed twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, hop, length, batch = 256, 64, 5 * 256, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randn(batch, length, dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    w = 0.5 + torch.rand(n, dtype=torch.float32, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = make(fa, "f32", n, hop)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.forward(xs[0])
        other.welch(xs[0])
    side.synchronize()
    plan = make(fa, "f32", n, hop)
    plan.set_option("fusion", fusion)
    plan.set_window(w)
    assert plan.describe().startswith("spectrogram fused rows" if fusion else "spectrogram composed"), plan.describe()
    plan.reserve(length, batch)
    nf = plan.frames(length)
    torch.cuda.synchronize()
    d = xs[0].clone()
    S = torch.empty(batch, nf, plan.bins(), dtype=torch.float32, device="cuda")
    P = torch.empty(batch, plan.bins(), dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(d, out=S)  # the first calls on this plan: captured
        plan.welch(d, out=P)
    wh = w.cpu().numpy()
    for x in xs[1:]:
        d.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eS, eP = plan.forward(x), plan.welch(x)
        torch.cuda.synchronize()
        assert torch.equal(S, eS) and torch.equal(P, eP), fusion
        assert rel_l2(S.cpu().numpy(), truth.spectrogram(x.cpu().numpy(), n, hop, n, wh, "reflect")) <= tol(plan, "f32")
        assert rel_l2(P.cpu().numpy(), truth.welch(x.cpu().numpy(), n, hop, n, wh, "reflect")) <= tol(plan, "f32")


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    for dt, real in ((torch.float32, "f32"), (torch.float64, "f64")):
        base = 2e-6 if real == "f32" else 1e-13
        n, hop = 512, 128
        x = torch.randn(2, 3, 2000, dtype=dt, device="cuda", generator=g)
        w = torch.hann_window(400, dtype=dt, device="cuda")
        nf = 1 + 2000 // hop
        for power in (1.0, 2.0):
            S = fa.spectrogram(x, n, hop, win_length=400, window=w, power=power, normalized=True)
            assert S.shape == (2, 3, nf, n // 2 + 1) and S.dtype == dt and S.is_contiguous()  # leading dimensions folded and restored
            want = truth.spectrogram(x.reshape(6, 2000).cpu().numpy(), n, hop, 400, w.cpu().numpy(), "reflect", int(power), True)
            assert rel_l2(S.reshape(6, nf, -1).cpu().numpy(), want) <= 4 * base
        ref = torch.stft(x.reshape(6, 2000), n, hop, 400, w, center=True, pad_mode="reflect", normalized=True, onesided=True,
                         return_complex=True).abs().square().transpose(-1, -2)
        assert rel_l2(S.reshape(6, nf, -1).cpu().numpy(), ref.cpu().numpy()) <= 8 * base  # two implementations, each within 4 x base
        assert fa.spectrogram(x[0, 0], 256).shape == (1 + 2000 // 64, 129)               # defaults: hop n_fft // 4, a window of ones
        # welch: scipy's definition without detrending, against the truth
        for nperseg, noverlap, scaling, onesided, fs in ((256, None, "density", True, 48.0), (255, 100, "spectrum", True, 1.0),
                                                         (400, 0, "density", False, 2.0)):
            f, P = fa.welch(x, fs, None, nperseg, noverlap, scaling, onesided)
            nov = nperseg // 2 if noverlap is None else noverlap
            wh = torch.hann_window(nperseg, periodic=True, dtype=torch.float64).to(dt).numpy()
            want = truth.welch(x.reshape(6, 2000).cpu().numpy(), nperseg, nperseg - nov, nperseg, wh, "none", onesided,
                               truth.welch_scale(wh, fs, scaling))
            assert P.shape == (2, 3, nperseg // 2 + 1) and P.dtype == dt and f.shape == (nperseg // 2 + 1,)
            assert np.allclose(f.cpu().numpy(), np.arange(nperseg // 2 + 1) * fs / nperseg, rtol=1e-6)
            err = rel_l2(P.reshape(6, -1).cpu().numpy(), want)
            assert err <= tol(fa.Spectrogram(nperseg, real, nperseg - nov, center=False, device=0), real), (real, nperseg, err)
        wt = 0.5 + torch.rand(256, dtype=dt, device="cuda", generator=g)
        f, P = fa.welch(x, 8.0, wt, 256, 192, "spectrum")
        want = truth.welch(x.reshape(6, 2000).cpu().numpy(), 256, 64, 256, wt.cpu().numpy(), "none", True,
                           truth.welch_scale(wt.cpu().numpy(), 8.0, "spectrum"))
        assert rel_l2(P.reshape(6, -1).cpu().numpy(), want) <= 4 * base
        # out= on the handle
        plan = fa.Spectrogram(n, real, hop, 400, device=0)
        plan.set_window(w)
        out = torch.empty(6, nf, n // 2 + 1, dtype=dt, device="cuda")
        assert plan.forward(x.reshape(6, 2000), 2, True, out=out) is out and torch.equal(out, S.reshape(6, nf, -1))
        with pytest.raises(TypeError):
            plan.forward(x.reshape(6, 2000), out=torch.empty(6, nf, n // 2 + 1, dtype=dt))
        with pytest.raises(ValueError):
            plan.forward(x, power=3)
    x = torch.randn(4, 1000, device="cuda")
    with pytest.raises(TypeError):
        fa.spectrogram(x.cpu(), 256)
    with pytest.raises(TypeError):
        fa.spectrogram(x.to(torch.complex64), 256)
    with pytest.raises(TypeError):
        fa.spectrogram(x, 256, window=torch.ones(256, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fa.spectrogram(x, 256, window=torch.ones(255, device="cuda"))
    with pytest.raises(ValueError):
        fa.spectrogram(x, 256, win_length=257)
    with pytest.raises(ValueError):
        fa.spectrogram(x, 256, hop_length=0)
    with pytest.raises(ValueError):
        fa.spectrogram(x, 256, pad_mode="edge")
    with pytest.raises(ValueError):
        fa.spectrogram(x, 256, power=0.5)
    with pytest.raises(ValueError):
        fa.spectrogram(x[:, :100], 256)          # reflect needs more than n_fft / 2 samples
    with pytest.raises(TypeError):
        fa.welch(x.cpu())
    with pytest.raises(ValueError):
        fa.welch(x, nperseg=2000)                # longer than the rows
    with pytest.raises(ValueError):
        fa.welch(x, nperseg=256, noverlap=256)
    with pytest.raises(ValueError):
        fa.welch(x, scaling="psd")
    with pytest.raises(ValueError):
        fa.welch(x, fs=0.0)
    with pytest.raises(ValueError):
        fa.welch(x, window=torch.ones(100, device="cuda"))
