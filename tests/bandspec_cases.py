"""The cases of the band-spectrogram handle (fourier_hip_bandspec_*, fourier_amd.BandSpectrogram), stated once and run twice: on the CPU
emulation (tests/test_bandspec_emu.py) and on the MI355X (tests/test_gpu_bandspec.py).  The two callers hand in an adapter (`api`):
  api.make(real, n_fft, bands, hop, win_length, pad_mode)  a BandSpectrogram
  api.upload(array)                                        a numpy array as device memory
  api.set_window(plan, d_window)
  api.forward(plan, d_x, batch, length, power, normalized, log_mult, log_floor)
      runs forward into a buffer that starts on an ODD element with a sentinel on both sides, checks the sentinels and returns the
      (batch, frames, bands) result as a numpy array
Everything else -- shapes, banks, assertions, tolerances -- is here.

Shapes: n_fft = 256 and the largest fused length (2048 at f32, 1024 at f64), frames = tile + 3 per row (TILE of
tests/test_gpu_spectrogram.py: the last workgroup is partly empty and tiles straddle rows), batch 3, even and odd hops and lengths, the
three pad modes, one win_length < n_fft, one case of 6 tile + 3 frames (more than 8 workgroups, no multiple of 8), and the composed-only
lengths 400 and 255.  Each case runs at both "fusion" values and both powers, linear and under the log.

Tolerances.  Linear output: relative L2 against tests/bandspec_truth.py at most tol() of tests/test_gpu_spectrogram.py.  The input is
white Gaussian and the mel weights are non-negative, so a band's relative error does not exceed its terms' error; the accumulation adds
at most width * eps / 2, below that tolerance at these widths.  A bank with negative entries: the same bound against the norm of
|W| @ S of the truth in place of the truth's own norm -- the terms of a band are not of one sign, so the sum can cancel while each
term's error does not (the reason tests/chunk_walks.py gives for the cross spectrum).  Log output: exp(out / log_mult) against
maximum(truth, floor) under the same relative L2 (the rounding of log_mult * ln(y) moves y by eps |ln y|, far inside the bound);
log_floor is the median of the truth's values, so about half of them clamp; an all-zero row must equal T(log_mult) * ln(T(floor)) to one
rounding: the product's half ulp, on a logarithm within one ulp of T of the exact one (taken in extended precision) -- what the library
logarithm delivers and a fast intrinsic does not.
Every figure is printed before it is asserted."""
import math

import numpy as np

import bandspec_truth as truth

# restated from tests/test_gpu_spectrogram.py (the same inner plans and frame kernels): frames per workgroup of the fused kernel at f32,
# half as many at f64, and tol(): twice the forward tolerance tests/test_gpu_stft.py's tol() gives the same inner plan and precision
TILE = {128: 32, 256: 64, 512: 32, 1024: 16, 2048: 8}


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return 2 * 2 * base


LOG_MULT = 10.0 / math.log(10.0)  # dB of a power


def np_real(real):
    return np.float32 if real == "f32" else np.float64


def largest_fused(real):
    return 2048 if real == "f32" else 1024


def has_fused(real, n_fft):
    return n_fft in (128, 256, 512, 1024) or (n_fft == 2048 and real == "f32")


def cols(real, n_fft):
    return TILE.get(n_fft, 32) // (1 if real == "f32" else 2)


def length_for(frames, n_fft, hop, pad_mode, extra):
    """a row length that gives `frames` frames, `extra` samples beyond the last frame's start rule"""
    return (frames - 1) * hop + extra + (n_fft if pad_mode == "none" else 0)


def mel_bank(n_fft, n_mels=None):
    """40 bands at n_fft 256 (and the composed-only lengths), 128 at the largest fused length; 16 kHz"""
    import fourier_amd

    n_mels = n_mels or (128 if n_fft >= 1024 else 40)
    return fourier_amd.mel_filterbank(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000.0, None, "htk")


def bank(kind, n_fft, seed=0):
    """The banks of the issue by name."""
    bins = n_fft // 2 + 1
    rng = np.random.default_rng(seed + bins)
    if kind == "mel":
        return mel_bank(n_fft)
    if kind == "dense":      # a random dense matrix with negative entries
        return rng.standard_normal((24, bins))
    if kind == "edges":      # an all-zero row, a row at bin 0 only, a row at the Nyquist bin only, a row over all bins -- in this order
        W = np.zeros((4, bins))
        W[1, 0] = 0.75
        W[2, bins - 1] = 1.25
        W[3] = 0.5 + rng.random(bins)
        return W
    if kind == "one":        # bands = 1
        return (0.5 + rng.random((1, bins))) * (np.arange(bins) % 3 != 1)  # zeros inside the support
    if kind == "odd":        # 37 bands: output rows only element-aligned
        return mel_bank(n_fft, 37)
    if kind in ("bins", "bins+1"):  # the fused route's limit and one beyond it: a signed band matrix of width 5 (wider in the corners)
        bands = bins if kind == "bins" else bins + 1
        W = np.zeros((bands, bins))
        for j in range(bands):
            lo, hi = max(0, min(j, bins - 1) - 2), min(bins, min(j, bins - 1) + 3)
            W[j, lo:hi] = rng.standard_normal(hi - lo)
        return W
    raise ValueError(kind)


def check(api, real, n_fft, hop, pad_mode="reflect", extra=3, batch=3, win_length=None, frames=None, kind="mel"):
    W = bank(kind, n_fft)
    W = W.astype(np_real(real)).astype(np.float64)  # what the handle holds: the truth uses the rounded weights
    bands, bins = W.shape
    signed = bool((W < 0).any())
    plan = api.make(real, n_fft, bands, hop, win_length, pad_mode)
    assert (plan.n_fft(), plan.hop(), plan.bins(), plan.bands()) == (n_fft, hop, bins, bands)
    plan.set_bands(W)
    frames = cols(real, n_fft) + 3 if frames is None else frames
    length = length_for(frames, n_fft, hop, pad_mode, extra)
    rng = np.random.default_rng(n_fft + hop + length)
    wh = np.ascontiguousarray((0.5 + rng.random(plan.win_length())).astype(np_real(real)))
    xh = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(np_real(real)))
    api.set_window(plan, api.upload(wh))
    dx = api.upload(xh)
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) == frames
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        fused = fusion == 1 and has_fused(real, n_fft) and bands <= bins
        route = "fused rows" if fused else "composed"
        d = plan.describe()
        assert d.startswith(f"bandspec {route}: real "), d
        bound = tol(plan, real)
        for power in (1, 2):
            normalized = power == 1
            want = truth.band_spectrogram(xh, W, n_fft, hop, plan.win_length(), wh, pad_mode, power, normalized)
            scale = truth.abs_band_spectrogram(xh, W, n_fft, hop, plan.win_length(), wh, pad_mode, power, normalized) if signed else want
            out = api.forward(plan, dx, batch, length, power, normalized, 0.0, 0.0)
            err = np.linalg.norm(out - want) / np.linalg.norm(scale)
            print(f"bandspec {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} {kind} bands={bands} power={power} {route}: "
                  f"err {err:.3g} tol {bound:.3g}")
            assert err <= bound, (real, n_fft, hop, pad_mode, kind, power, route, err)
            if kind == "edges":
                assert np.all(out[..., 0] == 0), "the all-zero row"
                for j in (1, 2, 3):  # bin 0, the Nyquist bin (the kernel carries it apart from the rest), every bin
                    e = np.linalg.norm(out[..., j] - want[..., j]) / np.linalg.norm(want[..., j])
                    print(f"  row {j}: err {e:.3g}")
                    assert e <= bound, (real, n_fft, kind, power, route, j, e)
            got[fusion, power] = out
            # under the log: about half of the values clamp at the floor
            floor = float(np.median(want[want > 0])) if (want > 0).any() else 1.0
            lout = api.forward(plan, dx, batch, length, power, normalized, LOG_MULT, floor)
            back = np.exp(lout.astype(np.float64) / LOG_MULT)
            lwant = np.maximum(want, floor)
            lerr = np.linalg.norm(back - lwant) / np.linalg.norm(np.maximum(scale, floor))
            print(f"  log floor={floor:.3g} clamped {np.mean(want <= floor):.2f}: err {lerr:.3g} tol {bound:.3g}")
            assert lerr <= bound, (real, n_fft, hop, pad_mode, kind, power, route, "log", lerr)
            if kind == "edges":
                # the all-zero row: the kernel computes T(log_mult) * ln(T(floor)) in T with the library logarithm -- ONE rounding (the
                # product's, half an ulp of the value) on a logarithm that is within one ulp of T of ln(T(floor)), the accuracy logf /
                # log have and a fast intrinsic has not (near 1 its error is a fixed absolute one, many ulps of a small logarithm).
                # ln(T(floor)) is taken in extended precision, so the reference adds no error of its own.
                T = np_real(real)
                lg = np.log(np.longdouble(T(floor)))
                v = np.longdouble(T(LOG_MULT)) * lg
                zb = float(abs(T(LOG_MULT))) * float(np.spacing(T(abs(lg)))) + 0.5 * float(np.spacing(T(abs(v))))
                dev = float(np.max(np.abs(lout[..., 0].astype(np.longdouble) - v)))
                print(f"  all-zero row under the log: {dev:.3g} from {float(v):.9g}, bound {zb:.3g} (one ulp of it {float(np.spacing(T(abs(v)))):.3g})")
                assert dev <= zb, (real, n_fft, power, route, dev, zb)
    for power in (1, 2):  # the two routes agree within the tolerance
        scale = truth.abs_band_spectrogram(xh, W, n_fft, hop, plan.win_length(), wh, pad_mode, power, power == 1)
        assert np.linalg.norm(got[1, power] - got[0, power]) / np.linalg.norm(scale) <= tol(plan, real)
    return plan


def fused_shapes(api, real):
    for n in (256, largest_fused(real)):
        check(api, real, n, n // 4, "reflect", extra=2)        # even rows and hop: pairs of reals
        check(api, real, n, n // 8 + 1, "reflect", extra=3)    # an odd hop, an odd length: single reals
        check(api, real, n, n // 4, "constant", extra=5)       # zero padding, an odd length
        check(api, real, n, n // 4, "none", extra=6)           # no padding: every frame interior
    check(api, real, 256, 64, "reflect", extra=2, win_length=200)


def more_workgroups_than_xcds(api, real):
    """6 tiles + 3 frames a row, batch 3: ceil(3 * (6 tile + 3) / tile) = 19 workgroups (20 at a tile of 8 frames), above 8 and no
    multiple of 8: real_xcd_block gives the first XCDs one block more than the rest."""
    for n in (256, largest_fused(real)):
        frames = 6 * cols(real, n) + 3
        wgs = -(-3 * frames // cols(real, n))
        assert wgs == (20 if cols(real, n) == 8 else 19) and wgs > 8 and wgs % 8 != 0
        plan = check(api, real, n, n // 4, "reflect", extra=2, frames=frames)
        plan.set_option("fusion", 1)
        assert plan.describe().startswith("bandspec fused rows"), plan.describe()


def composed_only_shapes(api, real):
    for n, hop, pad_mode in ((400, 100, "reflect"), (400, 37, "none"), (255, 63, "reflect"), (255, 64, "constant")):
        plan = check(api, real, n, hop, pad_mode)
        plan.set_option("fusion", 1)
        assert plan.describe().startswith("bandspec composed"), plan.describe()


BANK_KINDS = ("dense", "edges", "one", "odd", "bins", "bins+1")


def banks(api, real, kind):
    for n in (256, largest_fused(real)):
        plan = check(api, real, n, n // 4, "reflect", extra=2, kind=kind)
        plan.set_option("fusion", 1)
        want = "bandspec composed" if kind == "bins+1" else "bandspec fused rows"  # bands = bins + 1: composed even with "fusion" = 1
        assert plan.describe().startswith(want), plan.describe()
