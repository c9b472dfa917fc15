"""The band-spectrogram handle on the MI355X: fourier_hip_bandspec_* through fourier_amd.BandSpectrogram and band_spectrogram /
mel_spectrogram / mfcc on torch tensors, against tests/bandspec_truth.py (f64 numpy on the rounded input).  The shapes, banks,
assertions and tolerances are those of tests/bandspec_cases.py, which the CPU twin tests/test_bandspec_emu.py runs too (it also covers
the argument checks, forward before set_bands, a NaN weight, a bad log_floor and the allocation-free property after reserve).  Here in
addition: input on an odd element, every fused instantiation ten times, graph capture on a side stream, one chunk walk through the
experiments library under a small scratch bound, and the torch layer.  Every figure is printed before it is asserted."""
import ctypes
import os

import numpy as np
import pytest

import bandspec_cases as cases
import bandspec_truth as truth
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


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test (tests/test_gpu_chunks.py's fixture, restated): a handle keeps the
    library it was created from, so the handles are created directly and never through the cached tensor entry points."""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


def rdtype(torch, real):
    return torch.float32 if real == "f32" else torch.float64


def make(fa, real, n_fft, bands, hop, win_length=None, pad_mode="reflect"):
    return fa.BandSpectrogram(n_fft, bands, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode, 0)


class DeviceApi:
    def __init__(self, torch, fa):
        self.torch, self.fa = torch, fa

    def make(self, real, n_fft, bands, hop, win_length=None, pad_mode="reflect"):
        return make(self.fa, real, n_fft, bands, hop, win_length, pad_mode)

    def upload(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def set_window(self, plan, w):
        plan.set_window(w)

    def forward(self, plan, x, batch, length, power, normalized, log_mult, log_floor):
        torch = self.torch
        frames, bands = plan.frames(length), plan.bands()
        count = batch * frames * bands
        before = x.clone()
        buf = torch.full((count + 3,), SENTINEL, dtype=x.dtype, device="cuda")
        out = buf[1:1 + count].view(batch, frames, bands)
        assert out.data_ptr() % (2 * out.element_size()) != 0  # the output starts on an odd element
        assert plan.forward(x, power, normalized, log_mult, log_floor, out=out) is out
        res = out.cpu().numpy()
        assert buf[0].item() == SENTINEL and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the output was written"
        assert torch.equal(x, before), "forward modified its input"
        return res


@pytest.fixture(scope="module")
def api(torch, fa):
    return DeviceApi(torch, fa)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(api, real):
    cases.fused_shapes(api, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_xcds(api, real):
    cases.more_workgroups_than_xcds(api, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(api, real):
    cases.composed_only_shapes(api, real)


@pytest.mark.parametrize("kind", cases.BANK_KINDS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_banks(api, real, kind):
    cases.banks(api, real, kind)


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_input_on_an_odd_element(torch, fa, real, fusion):
    """An even hop, padding and row length: only the base address decides whether the fused kernel loads pairs of reals.  Rows that
    start one element into their allocation against the truth, and bit-equal to what the same handle gives from an aligned copy of
    them; the input buffer itself untouched."""
    dt = rdtype(torch, real)
    for n in (256, cases.largest_fused(real)):
        hop, batch = n // 4, 3
        frames = cases.cols(real, n) + 3
        length = cases.length_for(frames, n, hop, "reflect", 2)
        assert hop % 2 == 0 and length % 2 == 0
        g = torch.Generator(device="cuda").manual_seed(n + fusion)
        holder = torch.randn(batch * length + 2, dtype=dt, device="cuda", generator=g)
        before = holder.clone()
        x = holder[1:-1].view(batch, length)
        xa = x.clone()
        assert x.data_ptr() % (2 * x.element_size()) != 0 and xa.data_ptr() % (2 * x.element_size()) == 0
        W = cases.mel_bank(n).astype(cases.np_real(real)).astype(np.float64)
        plan = make(fa, real, n, W.shape[0], hop)
        w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
        plan.set_window(w)
        plan.set_bands(W)
        plan.set_option("fusion", fusion)
        assert plan.describe().startswith("bandspec fused rows" if fusion else "bandspec composed"), plan.describe()
        assert plan.frames(length) == frames
        xh, wh = xa.cpu().numpy(), w.cpu().numpy()
        for power, normalized in ((2, False), (1, True)):
            got, aligned = plan.forward(x, power, normalized), plan.forward(xa, power, normalized)
            err = rel_l2(got.cpu().numpy(), truth.band_spectrogram(xh, W, n, hop, n, wh, "reflect", power, normalized))
            print(f"bandspec odd input {real} n_fft={n} fusion={fusion} power={power}: err {err:.3g} tol {cases.tol(plan, real):.3g}")
            assert err <= cases.tol(plan, real), (real, n, fusion, power, err)
            assert torch.equal(got, aligned), (real, n, fusion, power)
        assert torch.equal(holder, before), "a call modified its input"


@pytest.mark.parametrize("n_fft", [128, 256, 512, 1024, 2048])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_results_are_repeatable(torch, fa, real, n_fft):
    """Every fused instantiation, both powers, ten times into fresh outputs: bit-equal to the first (a race on the kernel's LDS
    buffers shows as a difference between runs), and the first within tolerance of the truth.  Where the precision has no fused
    kernel of the length the composed route runs."""
    n, hop = n_fft, n_fft // 4
    g = torch.Generator(device="cuda").manual_seed(n)
    dt = rdtype(torch, real)
    frames, batch = cases.cols(real, n) + 3, 3
    length = cases.length_for(frames, n, hop, "reflect", 3)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    W = cases.mel_bank(n).astype(cases.np_real(real)).astype(np.float64)
    plan = make(fa, real, n, W.shape[0], hop)
    plan.set_bands(W)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("bandspec fused rows" if cases.has_fused(real, n) else "bandspec composed"), plan.describe()
    runs = [(plan.forward(x, 2), plan.forward(x, 1), plan.forward(x, 2, False, 1.0, 1e-3)) for _ in range(10)]
    torch.cuda.synchronize()
    for k, power in ((0, 2), (1, 1)):
        err = rel_l2(runs[0][k].cpu().numpy(), truth.band_spectrogram(x.cpu().numpy(), W, n, hop, pad_mode="reflect", power=power))
        print(f"bandspec repeat {real} n_fft={n} power={power}: err {err:.3g} tol {cases.tol(plan, real):.3g}")
        assert err <= cases.tol(plan, real), (real, n, power, err)
    for i, run in enumerate(runs[1:]):
        assert all(torch.equal(a, b) for a, b in zip(run, runs[0])), (real, n, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """forward, linear and under the log, captured on a side stream as the first calls of a handle that reserved (they must not
    allocate), one linear graph, replayed twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, hop, length, batch = 256, 64, 5 * 256, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randn(batch, length, dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    w = 0.5 + torch.rand(n, dtype=torch.float32, device="cuda", generator=g)
    W = cases.mel_bank(n).astype(np.float32).astype(np.float64)
    side = torch.cuda.Stream()
    other = make(fa, "f32", n, 40, hop)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_bands(W)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.forward(xs[0])
    side.synchronize()
    plan = make(fa, "f32", n, 40, hop)
    plan.set_option("fusion", fusion)
    plan.set_window(w)
    plan.set_bands(W)
    assert plan.describe().startswith("bandspec fused rows" if fusion else "bandspec composed"), plan.describe()
    plan.reserve(length, batch)
    nf = plan.frames(length)
    torch.cuda.synchronize()
    d = xs[0].clone()
    Y = torch.empty(batch, nf, 40, dtype=torch.float32, device="cuda")
    Z = torch.empty(batch, nf, 40, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(d, out=Y)  # the first calls on this plan: captured
        plan.forward(d, 1, True, cases.LOG_MULT, 0.25, out=Z)
    wh = w.cpu().numpy()
    for x in xs[1:]:
        d.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eY, eZ = plan.forward(x), plan.forward(x, 1, True, cases.LOG_MULT, 0.25)
        torch.cuda.synchronize()
        assert torch.equal(Y, eY) and torch.equal(Z, eZ), fusion
        assert rel_l2(Y.cpu().numpy(), truth.band_spectrogram(x.cpu().numpy(), W, n, hop, n, wh, "reflect")) <= cases.tol(plan, "f32")
        lin = truth.band_spectrogram(x.cpu().numpy(), W, n, hop, n, wh, "reflect", 1, True)
        assert rel_l2(np.exp(Z.cpu().numpy().astype(np.float64) / cases.LOG_MULT), np.maximum(lin, 0.25)) <= cases.tol(plan, "f32")


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_under_a_small_scratch_bound(torch, fx, monkeypatch, real):
    """Scratch bytes per frame of the composed route: bins complex + n_fft reals.  n_fft 250 (h = 125: with an odd number of frames per
    chunk the windowed frames start 8 bytes off a 16-byte boundary in f32), 35 frames a row, batch 3: bounds of 1, 3, 20 and 40 frames
    cut the 105 frames into 105, 35, 6 and 3 chunks, ending inside rows.  No sum crosses a frame: bit-equal to the unbounded handle of
    the same library on the same buffers, which is within tolerance of the truth."""
    n, hop, frames, batch, bands = 250, 61, 35, 3, 30
    dt = rdtype(torch, real)
    length = cases.length_for(frames, n, hop, "reflect", 3)
    g = torch.Generator(device="cuda").manual_seed(250)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
    W = cases.mel_bank(n, bands).astype(cases.np_real(real)).astype(np.float64)
    per_frame = (n // 2 + 1) * (8 if real == "f32" else 16) + n * (4 if real == "f32" else 8)

    def run(plan):
        plan.set_window(w)
        plan.set_bands(W)
        plan.set_option("fusion", 0)
        assert plan.describe().startswith("bandspec composed") and plan.frames(length) == frames
        count = batch * frames * bands
        outs = []
        for args in ((2, False, 0.0, 0.0), (1, True, cases.LOG_MULT, 0.5)):
            buf = torch.full((count + 128,), SENTINEL, dtype=dt, device="cuda")
            out = buf[64:64 + count].view(batch, frames, bands)
            plan.forward(x, *args, out=out)
            torch.cuda.synchronize()
            assert torch.all(buf[:64] == SENTINEL).item() and torch.all(buf[-64:] == SENTINEL).item(), "a guard element was written"
            outs.append(out.clone())
        return outs

    ref = run(make(fx, real, n, bands, hop))
    err = rel_l2(ref[0].cpu().numpy(), truth.band_spectrogram(x.cpu().numpy(), W, n, hop, n, w.cpu().numpy(), "reflect"))
    print(f"bandspec chunks {real}: unbounded err {err:.3g} tol {cases.tol(make(fx, real, n, bands, hop), real):.3g}")
    assert err <= cases.tol(make(fx, real, n, bands, hop), real)
    for k in (1, 3, 20, 40):
        assert k * per_frame < batch * frames * per_frame  # the bound is below the call's scratch (that the library honours it is observed by the CPU twin, through the emulator's allocator)
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(k * per_frame))
        try:
            small = make(fx, real, n, bands, hop)
        finally:
            monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        got = run(small)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (real, k)


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    sr = 16000
    for dt, real in ((torch.float32, "f32"), (torch.float64, "f64")):
        base = 2e-6 if real == "f32" else 1e-13
        n, hop, mels = 512, 128, 40
        x = torch.randn(2, 3, 2000, dtype=dt, device="cuda", generator=g)
        xh = x.reshape(6, 2000).cpu().numpy()
        w = torch.hann_window(400, dtype=dt, device="cuda")
        wh = w.cpu().numpy()
        nf = 1 + 2000 // hop
        W = fa.mel_filterbank(n // 2 + 1, 20.0, 7600.0, mels, sr, "slaney", "slaney")
        Wr = W.astype(cases.np_real(real)).astype(np.float64)
        for power in (1.0, 2.0):
            M = fa.mel_spectrogram(x, sr, n, mels, 20.0, 7600.0, hop, 400, w, power=power, normalized=True, norm="slaney", mel_scale="slaney")
            assert M.shape == (2, 3, nf, mels) and M.dtype == dt and M.is_contiguous()  # leading dimensions folded and restored
            want = truth.band_spectrogram(xh, Wr, n, hop, 400, wh, "reflect", int(power), True)
            err = rel_l2(M.reshape(6, nf, mels).cpu().numpy(), want)
            print(f"mel_spectrogram {real} power={power}: err {err:.3g} tol {4 * base:.3g}")
            assert err <= 4 * base
            # against the caller's composition, spectrogram(...) @ W.T: two implementations, each within the tolerance
            S = fa.spectrogram(x, n, hop, win_length=400, window=w, power=power, normalized=True)
            comp = S @ torch.from_numpy(W).to(dt).cuda().T
            assert rel_l2(M.cpu().numpy(), comp.cpu().numpy()) <= 2 * 4 * base
            B = fa.band_spectrogram(x, W, n, hop, 400, w, power=power, normalized=True)
            assert torch.equal(B, M)
        # dB, ln and log10 are compared element by element, so every element has a bound of its own.  The forward STFT of a frame is
        # off by at most tol_f = 2 * base times the frame's norm (tests/test_gpu_stft.py): ||dX|| <= tol_f sqrt(E_f), E_f = sum_k |X_k|^2.
        # A band moves by |dY_j| <= sum_k W[j, k] 2 |X_k| |dX_k| <= 2 sqrt(sum_k W[j, k]^2 |X_k|^2) ||dX|| (Cauchy-Schwarz), and a floored
        # value is at least max(Y, amin): its relative error is at most r[f, j] = 2 tol_f sqrt((W^2 @ S)[f, j] E_f) / max(Y[f, j], amin).
        # The logarithm turns that into an absolute error of r (ln), r / ln 10 (log10) or 10 / ln 10 * r (dB); its own rounding, the
        # multiplier's and the ref offset's add a few eps of the value: 16 eps |value| covers them.
        S2 = truth.spectrogram_truth.spectrogram(xh, n, hop, 400, wh, "reflect", 2, False)
        lin = S2 @ Wr.T
        amin = float(np.median(lin))
        r = 2 * (2 * base) * np.sqrt((S2 @ (Wr * Wr).T) * S2.sum(axis=-1, keepdims=True)) / np.maximum(lin, amin)
        eps16 = 16 * float(np.finfo(cases.np_real(real)).eps)
        for ref_, top_db in ((1.0, None), (3.5, 30.0)):
            D = fa.mel_spectrogram(x, sr, n, mels, 20.0, 7600.0, hop, 400, w, norm="slaney", mel_scale="slaney", log="db", amin=amin, ref=ref_,
                                   top_db=top_db)
            assert D.shape == (2, 3, nf, mels)
            Dh = D.reshape(6, nf, mels).cpu().numpy().astype(np.float64)
            want = truth.to_db(lin, 2, amin, ref_, top_db)
            bound = 10 / np.log(10) * r + eps16 * (np.abs(want) + abs(10 * np.log10(ref_)))
            if top_db is not None:  # a clamped element sits at its item's maximum minus top_db: it carries the bound of that maximum
                peak = np.take_along_axis(bound.reshape(6, -1), truth.to_db(lin, 2, amin, ref_).reshape(6, -1).argmax(axis=1)[:, None], 1)
                bound = np.maximum(bound, peak[:, :, None])
                assert np.all(Dh.min(axis=(-2, -1)) >= Dh.max(axis=(-2, -1)) - top_db * (1 + eps16))
            worst = float(np.max(np.abs(Dh - want) / bound))
            print(f"mel dB {real} ref={ref_} top_db={top_db}: max dev {np.max(np.abs(Dh - want)):.3g}, largest dev / bound {worst:.3g} "
                  f"(bounds {bound.min():.3g} ... {bound.max():.3g})")
            assert worst <= 1
        for log, f, c in (("ln", np.log, 1.0), ("log10", np.log10, 1 / np.log(10))):
            Lg = fa.mel_spectrogram(x, sr, n, mels, 20.0, 7600.0, hop, 400, w, norm="slaney", mel_scale="slaney", log=log, amin=amin)
            want = f(np.maximum(lin, amin))
            bound = c * r + eps16 * np.abs(want) + eps16 * c  # (a value near zero: the rounding of ln near 1 is absolute)
            worst = float(np.max(np.abs(Lg.reshape(6, nf, mels).cpu().numpy() - want) / bound))
            print(f"mel {log} {real}: largest dev / bound {worst:.3g} (bounds {bound.min():.3g} ... {bound.max():.3g})")
            assert worst <= 1
        # mfcc against the truth's DCT-II of the truth's dB mel spectrogram.  The orthonormal DCT's rows have unit norm, so a coefficient
        # moves by at most the L2 norm of the errors of its frame's dB values -- the norm of that frame's bounds above (with the
        # clamp's) -- and the transform itself adds tests/test_gpu_r2r.py's tolerance, 2 * base, times the L2 norm of the frame.
        C = fa.mfcc(x, sr, 13, n, mels, 20.0, 7600.0, hop, 400, w, mel_scale="slaney", mel_norm="slaney", amin=amin, top_db=80.0)
        assert C.shape == (2, 3, nf, 13) and C.is_contiguous()
        db = truth.to_db(lin, 2, amin, 1.0, 80.0)
        dbb = 10 / np.log(10) * r + eps16 * np.abs(db)
        peak = np.take_along_axis(dbb.reshape(6, -1), truth.to_db(lin, 2, amin, 1.0).reshape(6, -1).argmax(axis=1)[:, None], 1)
        dbb = np.maximum(dbb, peak[:, :, None])
        want = truth.dct2(db, "ortho")[..., :13]
        bound = (np.linalg.norm(dbb, axis=-1) + 2 * base * np.linalg.norm(db, axis=-1))[..., None]
        dev = np.abs(C.reshape(6, nf, 13).cpu().numpy() - want)
        print(f"mfcc {real}: max dev {dev.max():.3g}, largest dev / bound {float(np.max(dev / bound)):.3g} "
              f"(bounds {bound.min():.3g} ... {bound.max():.3g})")
        assert np.all(dev <= bound)
        assert fa.mel_spectrogram(x[0, 0], sr, 256, 20).shape == (1 + 2000 // 64, 20)   # defaults: hop n_fft // 4, a window of ones
        # out= on the handle
        plan = fa.BandSpectrogram(n, mels, real, hop, 400, device=0)
        plan.set_window(w)
        plan.set_bands(torch.from_numpy(W))  # a torch tensor on the host; a CUDA tensor works too
        out = torch.empty(6, nf, mels, dtype=dt, device="cuda")
        assert plan.forward(x.reshape(6, 2000), 2, True, out=out) is out and torch.equal(out, M.reshape(6, nf, mels))
        plan.set_bands(torch.from_numpy(W).cuda())
        assert torch.equal(plan.forward(x.reshape(6, 2000), 2, True), out)
        with pytest.raises(TypeError):
            plan.forward(x.reshape(6, 2000), out=torch.empty(6, nf, mels, dtype=dt))
        with pytest.raises(ValueError):
            plan.forward(x, power=3)
        with pytest.raises(ValueError):
            plan.forward(x, log_mult=1.0, log_floor=0.0)
        with pytest.raises(fa.FourierError):
            fa.BandSpectrogram(n, mels, real, hop, 400, device=0).forward(x)  # no bank yet
    x = torch.randn(4, 1000, device="cuda")
    W = fa.mel_filterbank(129, 0.0, 8000.0, 20, sr)
    with pytest.raises(TypeError):
        fa.mel_spectrogram(x.cpu(), sr, 256)
    with pytest.raises(TypeError):
        fa.mel_spectrogram(x.to(torch.complex64), sr, 256)
    with pytest.raises(TypeError):
        fa.mel_spectrogram(x, sr, 256, window=torch.ones(256, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, window=torch.ones(255, device="cuda"))
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, win_length=257)
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, hop_length=0)
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, pad_mode="edge")
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, power=0.5)
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x[:, :100], sr, 256)      # reflect needs more than n_fft / 2 samples
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, log="dB")
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, log="db", amin=0.0)
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, log="ln", top_db=80.0)
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, mel_scale="bark")
    with pytest.raises(ValueError):
        fa.mel_spectrogram(x, sr, 256, f_min=9000.0)
    with pytest.raises(ValueError):
        fa.band_spectrogram(x, W[:, :100], 256)
    with pytest.raises(TypeError):
        fa.band_spectrogram(x, W.tolist(), 256)
    with pytest.raises(ValueError):
        fa.mfcc(x, sr, 50, 256, 40)
