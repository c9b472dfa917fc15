"""The library across the amplitude range: one table of cases, stated once and run twice -- on the CPU emulation
(tests/test_amplitude_emu.py) and on the MI355X (tests/test_gpu_amplitude.py).  Every other accuracy test feeds unit-variance noise and
measures a relative L2 error, which says nothing about scale; these cases feed the same kernels 2^k x and integer-valued samples.

The two callers hand in an adapter (`api`):
  api.fa, api.device          fourier_amd bound to the library under test, the device index the handles are created on
  api.put(array), api.ptr(b)  a numpy array as memory of the library's side, and its address
  api.run(call, shape, dtype) runs call(address of an output of `shape` between guard elements), checks the guards, returns numpy
Everything else -- shapes, routes, inputs, assertions, tolerances -- is here.

A case (Case below) is a constructor, the option settings that select each of its routes with the describe() prefix the route must
show (a silent fall-back fails there), the degree d of the output in the input amplitude, a maker of unit-variance Gaussian inputs from
a seeded numpy generator, a runner through the handle's *_ptr entry point and the family's f64 truth (tests/*_truth.py, numpy for the
core).  Shapes are the smallest that reach each kernel family (a partly empty last tile, more than one workgroup), batch 3, f32 and f64.

The families: the core plans, real / N-D / strided-axis / DCT-DST transforms, circular and linear convolution, STFT, MDCT, the filter
banks, resampling, chirp-z, analytic signal and envelope, power / magnitude / Welch spectrogram, cross spectrum and coherence, band
spectrogram; cross-correlation and GCC-PHAT, fractional delay and delay-and-sum, N-D convolution, the non-uniform FFT, cepstrum and
minimum phase.  The last five state their own conditions on the inputs (kappa of the PHAT and cepstrum rows, the f64 model of the
NUFFT) and assert them before anything runs.

Assertions (a test prints its worst figures in one line, then asserts every one of them):
  (a) exact scaling   with y0 = f(x): f(2^k x) is BIT-equal to 2^(k d) y0 over the whole output.  2^k x is formed in the working
                      precision, which is exact.  k by precision and degree is K below; these k keep every input, table product and
                      output of the cases normal with a wide margin, so a device that flushes subnormals changes nothing.
                      d = 1: the linear entry points; d = 2: power spectrogram, Welch, cross spectrum, band sums of powers; d = 0: the
                      coherence, whose k go past the point (2^28 in f32) where a product of two summed powers leaves the format, and
                      GCC-PHAT.  The bilinear cross-correlation also runs as the kind "opposite": x 2^k against y 2^-k at the k of
                      OPPOSITE, +-40 and +-100 (f64 +-300, +-900), net degree 0, so no bit of the output may change; 2^100 squared
                      is beyond FLT_MAX, which is what GCC-PHAT's composed route has to survive there.
  (b) truth           at k = 0 and at the largest and the smallest k of (a): relative L2 against the truth of the scaled, rounded input
                      within the tolerance the family's own GPU test grants (restated below from each tol(); none is new -- relative L2
                      does not change with scale).  A band spectrogram under the log has no degree: exp(out / log_mult) against
                      maximum(truth, floor) with the floor the median of the truth, the rule of tests/bandspec_cases.py.  The cepstrum
                      and the minimum-phase row have none either: tests/cepstrum_truth.py's err, which divides by kappa and does not
                      move with scale, at k = +-40 / +-300 under tests/cepstrum_cases.py's bound, and at EVERY k the identity that
                      the truths satisfy exactly -- c(2^k x) - k log_mult ln 2 at quefrency 0 against c(x), 2^(-k log_mult) h(2^k x)
                      against h(x) -- in the same measure under TWICE that bound (two results, each within one bound of its truth).
  (c) integers        f32 only: round(sigma gauss) clipped to the integer type -- sigma 2^13 as int16, 2^21 as int24, 2^28 as int32 --
                      through the power, magnitude and Welch spectrograms, cross spectrum and coherence, the band spectrogram in dB, the
                      envelope and the real transform, the cross-correlation (x alone; x and y, where int32 x int32 x n reaches
                      about 2^67), the delay, the N-D convolution's items, the NUFFT's strengths and modes (pairs of integers) and
                      the cepstrum (not the minimum-phase row, whose input is a filter), against the truth under the same
                      tolerances, every output finite; and two full-scale 24-bit tones
                      (two_tone below), whose coherence must be finite and within tolerance in the bins that hold the tone.
  (d) range edges     spectrogram magnitude and envelope are sqrt(re^2 + im^2): |X|^2 must be representable, |X| < sqrt(FLT_MAX) ~ 2^64
                      (f64: 2^512).  With k chosen so that max |y0| 2^k lies in [2^61, 2^62) (f64 [2^509, 2^510)) the output is finite
                      and exactly scaled.  The edge is derived from the format, not measured; include/fourier.h states it.  GCC-PHAT
                      and the cepstrum form re^2 + im^2 of the SPECTRUM: k places the largest |X[k]| of the scaled inputs' f64
                      spectra there; the PHAT output is bit-identical to k = 0 and finite, the cepstrum finite and within its bound.
                      Nothing is asserted at the lower edge: single bins of a spectrum can be arbitrarily small."""
import math
import re
import types

import numpy as np

import bandspec_truth
import cepstrum_cases
import cepstrum_truth
import convnd_cases
import convnd_truth
import csd_truth
import czt_truth
import delay_cases
import delay_truth
import hilbert_truth
import ipfb_truth
import mdct_truth
import nufft_cases
import nufft_truth
import pfb_truth
import r2r_truth
import resample_truth
import spectrogram_truth
import stft_truth
import xcorr_truth
from helpers import rel_l2

BATCH = 3
K = {"f32": {1: (-40, 40), 2: (-24, 24), 0: (-24, 24, 28, 40)},
     "f64": {1: (-300, 300), 2: (-150, 150), 0: (-150, 150)}}
OPPOSITE = {"f32": (-100, -40, 40, 100), "f64": (-900, -300, 300, 900)}  # (a), kind "opposite": x 2^k against y 2^-k
EDGE = {"f32": 61, "f64": 509}                       # (d): the binary exponent of the largest scaled magnitude
INTEGERS = ((13, 16), (21, 24), (28, 32))            # (c): log2 sigma, bits of the integer type
LOG_MULT = 10.0 / math.log(10.0)                     # dB of a power
FFT, IFFT, SQRT_IFFT = 0, 1, 4                       # fourier_amd.Transform
GUARD, SENTINEL = 64, 77.0


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


# ---- tolerances, restated from the families' GPU tests the way tests/test_gpu_chunks.py restates them
def base_tol(d, real):
    """tests/test_gpu_real.py's tol(): one transform of the inner plan"""
    blu = "bluestein" in d
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def times(factor):
    return lambda d, real: factor * base_tol(d, real)


def axis_tol(d, real):
    """tests/test_gpu_axis.py's tol()"""
    blu = "bluestein" in d
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-12)


def realnd_tol(d, real):
    """tests/test_gpu_realnd.py's tol() at rank 2"""
    return 2e-6 if real == "f32" else 1e-12


def czt_tol(d, real):
    """tests/czt_cases.py's bound on the unit circle (chirp ratio 1)"""
    return 4e-6 if real == "f32" else 1e-11


def csd_base(d, real):
    """tests/test_gpu_csd.py's base()"""
    blu = "bluestein" in d
    return (4e-6 if blu else 2e-6) if real == "f32" else (2e-13 if blu else 1e-13)


def csd_tol(d, real):
    return 4 * csd_base(d, real)


def coherence_tol(d, real):
    return 12 * csd_base(d, real)


# tests/test_gpu_r2r.py, _stft.py and _mdct.py (forward 2 x, inverse 4 x), _pfb.py, _ipfb.py, _resample.py, _hilbert.py: 2 x;
# _conv.py and _lconv.py: 3 x; _spectrogram.py and tests/bandspec_cases.py: 2 x 2 x
TWO, THREE, FOUR = times(2), times(3), times(4)


# ---- scaling and comparing
def scale(a, k):
    """2^k a in a's own precision: exact while the result is normal"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        return np.ldexp(a.view(a.real.dtype), k).view(a.dtype)
    return np.ldexp(a, k)


def differing(a, b):
    """the number of reals of a and b whose bits differ"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    u = np.uint32 if a.real.dtype == np.float32 else np.uint64
    return int(np.count_nonzero(np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)))


class HostApi:
    """the adapter of the CPU emulation build: `fa` is fourier_amd bound to it, the buffers are host memory"""
    device = -1

    def __init__(self, fa):
        self.fa = fa

    def put(self, a):
        return np.ascontiguousarray(a)

    def ptr(self, b):
        return b.ctypes.data

    def run(self, call, shape, dtype):
        count = int(np.prod(shape))
        buf = np.full(count + 2 * GUARD, SENTINEL, dtype)
        out = buf[GUARD:GUARD + count]
        out[:] = np.nan
        call(out.ctypes.data)
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL), "a guard element was written"
        return out.reshape(shape).copy()


class Case:
    """name; d: the degree (None: no exact scaling, `kd` picks the k of (b)); make(api, real) -> ctx with .plan; routes(real) ->
    ((options, describe prefix or compiled pattern), ...); inputs(ctx, rng) -> unit-variance f64 / c128 arrays; scaled: the inputs
    that carry the amplitude; run(api, ctx, ins) -> numpy; truth(ctx, ins) -> f64; pick(ctx, out): the part of out the truth covers;
    err(ctx, out, want): the figure held against tol(describe, real), or against bound(ctx, describe, real) where the family's bound
    depends on the inputs or on where the handle runs.
    signs: input -> +1 / -1, the sign of the exponent that input takes (the kind "opposite": x 2^k, y 2^-k; d counts the output's
    net degree, 0 there); ks: the exponents by precision where they are not K's; conditions(ctx, ins): the family's conditions on
    its inputs, asserted before anything runs; identity(ctx, k, scaled output, unscaled output, ins) -> a figure held against TWICE
    the bound at every k (a family with d = None whose truths scale by a known rule: the triangle inequality over two results);
    edge_of(ctx, ins, y0): the magnitude that (d) places at the range edge (default: the largest |y0|); hold(ctx, ins): fixes every
    parameter that run() derives from its inputs at its value for `ins`, for the later runs on ctx (tests/isolation_cases.py, whose
    poisoned inputs have no median: the log band spectrogram's floor)"""

    def __init__(self, name, d, make, routes, inputs, run, truth, tol, scaled=None, pick=None, err=None, kd=None, integers=False,
                 edge=False, describe=None, signs=None, ks=None, conditions=None, bound=None, identity=None, edge_of=None, hold=None):
        self.name, self.d, self.make, self.inputs, self.run, self.truth, self.tol = name, d, make, inputs, run, truth, tol
        self.routes = routes if callable(routes) else (lambda real: routes)
        self.scaled, self.pick, self.err = scaled, pick or (lambda ctx, out: out), err or (lambda ctx, out, want: rel_l2(out, want))
        self.kd = d if kd is None else kd
        self.integers, self.edge = integers, edge
        self.describe = describe or (lambda ctx: ctx.plan.describe())
        self.signs, self.ks_of = signs or {}, ks or (lambda real: K[real][self.kd])
        self.conditions = conditions or (lambda ctx, ins: None)
        self.bound = bound or (lambda ctx, d, real: self.tol(d, real))
        self.identity = identity
        self.edge_of = edge_of or (lambda ctx, ins, y0: float(np.max(np.abs(y0))))
        self.hold = hold or (lambda ctx, ins: None)

    def unit_inputs(self, ctx):
        return self.inputs(ctx, np.random.default_rng(sum(self.name.encode())))

    def carries(self, i):
        return self.scaled is None or i in self.scaled

    def at(self, ins, k):
        """the inputs at amplitude 2^k: every input that carries it, by the sign of its exponent"""
        return [scale(a, k * self.signs.get(i, 1)) if self.carries(i) else a for i, a in enumerate(ins)]

    def select(self, ctx, real, options, prefix):
        for key, value in options.items():
            ctx.plan.set_option(key, value)
        d = self.describe(ctx)
        ok = d.startswith(prefix) if isinstance(prefix, str) else prefix.match(d)
        assert ok, (self.name, real, options, d)
        return d


def rounded(ins, real):
    return [np.ascontiguousarray(a.astype(cdt(real) if np.iscomplexobj(a) else rdt(real))) for a in ins]


class Report:
    """the figures of one test: its worst ones are printed in ONE line, then everything is asserted"""

    def __init__(self, what):
        self.what, self.routes, self.bad, self.reals, self.notes, self.failed = what, [], 0, 0, [], []
        self.worst = (0.0, 0.0, 1.0, "")  # ratio, figure, bound, where

    def route(self, d):
        self.routes.append(d if not self.routes else d.split(":")[0].split(",")[0])  # the first describe() whole, the others by name

    def exact(self, where, got, want):
        bad = differing(got, want)
        self.bad, self.reals = self.bad + bad, self.reals + got.size * (2 if got.dtype.kind == "c" else 1)
        if bad:
            self.failed.append((where, f"{bad} reals differ from the exactly scaled result"))

    def figure(self, where, value, bound):
        ratio = value / bound if value == value else math.inf
        if ratio >= self.worst[0]:
            self.worst = (ratio, value, bound, where)
        if not value <= bound:
            self.failed.append((where, value, bound))

    def print(self):
        parts = [f"{self.bad} of {self.reals} reals differ from the exactly scaled result"] if self.reals else []
        if self.worst[3]:
            parts.append(f"worst error {self.worst[1]:.3g} of {self.worst[2]:.3g} ({self.worst[3]})")
        print(f"amplitude {self.what}: " + "; ".join(parts + self.notes) + f"  [{' | '.join(self.routes)}]")

    def check(self):
        assert not self.failed, (self.what, self.failed)


def opt(options):
    return "".join(f"{key}={value} " for key, value in options.items())


def figure(what, value, bound):
    print(f"amplitude {what}: figure {value:.3g} bound {bound:.3g}")
    assert value <= bound, (what, value, bound)


def check_scaling(api, case, real):
    """(a) and (b)"""
    ctx = case.make(api, real)
    ins = rounded(case.unit_inputs(ctx), real)
    case.conditions(ctx, ins)
    ks = case.ks_of(real)
    rep = Report(f"{real} {case.name}, k = {', '.join(f'{k:+d}' for k in ks)}")
    identity = (0.0, 0.0, 0.0, "")
    try:
        for options, prefix in case.routes(real):
            d = case.select(ctx, real, options, prefix)
            rep.route(d)
            t = case.bound(ctx, d, real)
            y0 = case.run(api, ctx, ins)
            rep.figure(f"{opt(options)}k=0", case.err(ctx, case.pick(ctx, y0), case.truth(ctx, ins)), t)
            for k in ks:
                sc = case.at(ins, k)
                y = case.run(api, ctx, sc)
                if case.d is not None:
                    rep.exact(f"{opt(options)}k={k:+d}", y, scale(y0, k * case.d))
                if case.identity is not None:
                    fig = case.identity(ctx, k, case.pick(ctx, y), case.pick(ctx, y0), ins)
                    identity = max(identity, (fig / (2 * t), fig, 2 * t, f"{opt(options)}k={k:+d}"))
                    rep.figure(f"{opt(options)}k={k:+d} against k=0", fig, 2 * t)
                if k in (min(ks), max(ks)):
                    rep.figure(f"{opt(options)}k={k:+d}", case.err(ctx, case.pick(ctx, y), case.truth(ctx, sc)), t)
    finally:
        if identity[3]:
            rep.notes.append(f"worst identity against k=0 {identity[1]:.3g} of {identity[2]:.3g} ({identity[3]})")
        rep.print()
    rep.check()


def integer_samples(ins, case, log2_sigma, bits):
    """round(sigma g) clipped to the integer type, as f32 (the inputs that carry no amplitude: rounded to f32 as they are); complex
    samples are a pair of integers"""
    lo, hi = -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1

    def ints(a):
        if np.iscomplexobj(a):
            return ints(a.real) + 1j * ints(a.imag)
        return np.clip(np.rint(2.0 ** log2_sigma * a), lo, hi)

    return [np.ascontiguousarray((ints(a) if case.carries(i) else a).astype(np.complex64 if np.iscomplexobj(a) else np.float32))
            for i, a in enumerate(ins)]


def check_integers(api, case):
    """(c): f32"""
    ctx = case.make(api, "f32")
    unit = case.unit_inputs(ctx)
    rep = Report(f"f32 {case.name}, int16 / int24 / int32 samples")
    try:
        for options, prefix in case.routes("f32"):
            d = case.select(ctx, "f32", options, prefix)
            rep.route(d)
            for log2_sigma, bits in INTEGERS:
                ins = integer_samples(unit, case, log2_sigma, bits)
                assert all(np.array_equal(a.view(np.float32), np.rint(a.view(np.float32))) for i, a in enumerate(ins) if case.carries(i))
                case.conditions(ctx, ins)
                y = case.run(api, ctx, ins)
                if not np.all(np.isfinite(y.view(np.float32))):
                    rep.failed.append((options, bits, f"{int(np.count_nonzero(~np.isfinite(y.view(np.float32))))} non-finite"))
                rep.figure(f"{opt(options)}int{bits}", case.err(ctx, case.pick(ctx, y), case.truth(ctx, ins)), case.bound(ctx, d, "f32"))
    finally:
        rep.print()
    rep.check()


def check_edge(api, case, real):
    """(d)"""
    ctx = case.make(api, real)
    ins = rounded(case.unit_inputs(ctx), real)
    case.conditions(ctx, ins)
    rep = Report(f"{real} {case.name}, range edge")
    try:
        for options, prefix in case.routes(real):
            d = case.select(ctx, real, options, prefix)
            rep.route(d)
            y0 = case.run(api, ctx, ins)
            largest = case.edge_of(ctx, ins, y0)
            k = EDGE[real] - int(math.floor(math.log2(largest)))
            top = math.ldexp(largest, k)
            assert 2.0 ** EDGE[real] <= top < 2.0 ** (EDGE[real] + 1), (k, top)
            sc = case.at(ins, k)
            y = case.run(api, ctx, sc)
            bad = int(np.count_nonzero(~np.isfinite(y)))
            rep.notes.append(f"{opt(options)}k={k:+d}: largest 2^{math.log2(top):.2f}, {bad} non-finite")
            if bad:
                rep.failed.append((options, k, f"{bad} non-finite"))
            if case.d is not None:
                rep.exact(f"{opt(options)}k={k:+d}", y, scale(y0, k * case.d))
            else:  # no exact scaling: within the family's bound of the truth at this amplitude
                rep.figure(f"{opt(options)}k={k:+d}", case.err(ctx, case.pick(ctx, y), case.truth(ctx, sc)), case.bound(ctx, d, real))
    finally:
        rep.print()
    rep.check()


# ---- the two-tone case of (c)
TONE = dict(n_fft=2048, hop=512, frames=9, bin=200, amplitude=8388607.0, phase=0.3, noise=50.0)


def two_tone(api):
    """Two full-scale 24-bit tones at bin 200 of n_fft 2048 (amplitudes 2^23 - 1 and half of it, phase 0.3) plus noise of sigma 50,
    rounded to integers, 9 frames, Hann window, f32, both routes.  The coherence in bins 199 ... 201 -- the ones a caller computes it
    for -- must be finite and within tests/test_gpu_csd.py's tol_coherence of the truth (0.964, 0.983, 0.951 in the first row, printed); no
    bin may be non-finite where the truth is finite.  The bins that hold only noise are not compared: their f32 frames carry the
    rounding of a tone 2^17 times larger."""
    n, hop, nb = TONE["n_fft"], TONE["hop"], TONE["bin"]
    length = (TONE["frames"] - 1) * hop + 2
    rng = np.random.default_rng(2048)
    t = np.arange(length)
    lo, hi = -2.0 ** 23, 2.0 ** 23 - 1
    x = TONE["amplitude"] * np.cos(2 * np.pi * nb / n * t) + TONE["noise"] * rng.standard_normal((BATCH, length))
    y = 0.5 * TONE["amplitude"] * np.cos(2 * np.pi * nb / n * t + TONE["phase"]) + TONE["noise"] * rng.standard_normal((BATCH, length))
    x, y = (np.ascontiguousarray(np.clip(np.rint(v), lo, hi).astype(np.float32)) for v in (x, y))
    w = stft_truth.hann(n, np.float32)
    plan = api.fa.CrossSpectrum(n, "f32", hop, None, True, "reflect", api.device)
    dw, dx, dy = api.put(w), api.put(x), api.put(y)
    plan.set_window_ptr(api.ptr(dw))
    assert plan.frames(length) == TONE["frames"]
    want = csd_truth.coherence(x, y, n, hop, n, w, "reflect")
    print("amplitude two-tone truth, row 0, bins 199 ... 201:", want[0, nb - 1:nb + 2])
    for fusion, route in ((1, "fused rows"), (0, "composed")):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        assert d.startswith(f"csd {route}, coherence {route}: real "), d
        got = api.run(lambda out: plan.coherence_ptr(api.ptr(dx), api.ptr(dy), out, length, BATCH), (BATCH, plan.bins()), np.float32)
        bad = int(np.count_nonzero(~np.isfinite(got) & np.isfinite(want)))
        print(f"amplitude two-tone {route}: {bad} non-finite bins where the truth is finite; bins 199 ... 201 of row 0: {got[0, nb - 1:nb + 2]}")
        assert bad == 0, (route, bad)
        figure(f"two-tone {route} bins 199 ... 201", rel_l2(got[:, nb - 1:nb + 2], want[:, nb - 1:nb + 2]), coherence_tol(d, "f32"))


# ---- inputs
def gauss(rng, *shape):
    return rng.standard_normal(shape)


def cgauss(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def half_spectrum(rng, rows, n):
    """the half spectrum of real Gaussian rows at unit variance (bin 0 and, n even, bin n / 2 are real)"""
    return np.fft.rfft(rng.standard_normal(rows + (n,)), axis=-1) / math.sqrt(n)


def window(rng, real, n):
    return np.ascontiguousarray((0.5 + rng.random(n)).astype(rdt(real)))


def ctx_of(plan, **kw):
    """the context of a case: the handle, the batch of the next call -- and, of a frame handle, its length and frame count (restate) --
    and of a convolution the number of filters (fftconv: and of taps) that run() sets, which inputs, run and truth read from here, so
    that a caller may state them per call (tests/history_cases.py); likewise `normalized` of the STFT and MDCT calls, the r2r norm, `onesided_fold` and `scale` of Welch and the cross spectrum, `correlate` of
    the 1-D convolutions, and the window and `filter_first` of the N-D convolution"""
    return types.SimpleNamespace(plan=plan, batch=BATCH, normalized=False, fold=True, scale=0.37, **kw)


def restate(c, length, nf):
    """the length and the frame count of the next call of a frame handle"""
    c.length, c.nf = length, nf
    return c


def fusion_routes(fused, composed, has=lambda real: True):
    """both "fusion" values where the fused route exists, else the composed one under "fusion" = 1 (which must stay composed)"""
    return lambda real: (({"fusion": 1}, fused), ({"fusion": 0}, composed)) if has(real) else (({"fusion": 1}, composed),)


CASES = []


def add(*args, **kw):
    CASES.append(Case(*args, **kw))


# ---- core plans
CORE = {64: "stockham 64 ", 4096: "stockham 64x64 one-launch ", 1000: "stockham mixed-radix 5.5.5.8 ",
        1001: "stockham registers 13x11x7 one-launch ", 1031: re.compile(r"bluestein M=\d+ registers \S+ one-launch "),
        255: re.compile(r"bluestein M=\d+ (inner \d+ fused|registers \S+ one-launch) "), 12288: "stockham mixed tiles 128x96 ",
        44100: "stockham mixed tiles 210x210 ", 16411: re.compile(r"bluestein M=\d+ inner mixed tiles \d+x\d+ "),
        65536: re.compile(r"stockham \d+x\d+(x\d+)? f")}
TWO_PASSES = re.compile(r"stockham \d+x\d+ f(32|64)$")  # two tile passes, not in one launch
CORE_TRUTH = {FFT: lambda x: np.fft.fft(x, axis=-1), IFFT: lambda x: np.fft.ifft(x, axis=-1),
              SQRT_IFFT: lambda x: np.fft.ifft(x, axis=-1) * math.sqrt(x.shape[-1])}


def smallest_two_passes(api, real):
    """the smallest power of two whose default plan is two tile passes, by describe()"""
    for log2n in range(6, 21):
        plan = api.fa.Fft(1 << log2n, real, api.device)
        if TWO_PASSES.match(plan.describe()):
            return plan
    raise AssertionError("no power of two up to 2^20 runs as two tile passes")


def core(n, code, name):
    def make(api, real):
        return ctx_of(api.fa.Fft(n, real, api.device) if n else smallest_two_passes(api, real))

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.transform_batch_ptr(api.ptr(x), out, c.batch, code), ins[0].shape, ins[0].dtype)

    add(f"fft {n or 'smallest two passes'} {name}", 1, make, (({}, CORE[n] if n else TWO_PASSES),), lambda c, rng: [cgauss(rng, c.batch, c.plan.size())],
        run, lambda c, ins: CORE_TRUTH[code](ins[0].astype(np.complex128)), base_tol)


for _n in (64, 4096, 1000, 1001, 1031, 255, 12288, 44100, 16411, 65536, 0):
    for _code, _name in ((FFT, "Fft"), (IFFT, "Ifft"), (SQRT_IFFT, "SqrtScaledIfft")):
        core(_n, _code, _name)


# ---- real transforms, N-D, a strided axis, DCT / DST
def rfft(n):
    def make(api, real):
        return ctx_of(api.fa.RealFft(n, real, api.device))

    def forward(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_batch_ptr(api.ptr(x), out, c.batch), (c.batch, n // 2 + 1), cdt(c.plan.real))

    def inverse(api, c, ins):
        s = api.put(ins[0])
        return api.run(lambda out: c.plan.inverse_batch_ptr(api.ptr(s), out, c.batch), (c.batch, n), rdt(c.plan.real))

    add(f"rfft {n}", 1, make, (({}, "real "),), lambda c, rng: [gauss(rng, c.batch, n)], forward,
        lambda c, ins: np.fft.rfft(ins[0].astype(np.float64), axis=-1), base_tol, integers=n == 4096)
    add(f"irfft {n}", 1, make, (({}, "real "),), lambda c, rng: [half_spectrum(rng, (c.batch,), n)], inverse,
        lambda c, ins: np.fft.irfft(ins[0].astype(np.complex128), n=n, axis=-1), base_tol)


for _n in (4096, 1001):
    rfft(_n)


def rfftn(shape):
    half = shape[:-1] + (shape[-1] // 2 + 1,)
    axes = tuple(range(1, len(shape) + 1))

    def make(api, real):
        return ctx_of(api.fa.RealFftN(shape, real, api.device))

    def forward(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_batch_ptr(api.ptr(x), out, c.batch), (c.batch,) + half, cdt(c.plan.real))

    def inverse(api, c, ins):
        s = api.put(ins[0])
        return api.run(lambda out: c.plan.inverse_batch_ptr(api.ptr(s), out, c.batch), (c.batch,) + shape, rdt(c.plan.real))

    add(f"rfftn {list(shape)}", 1, make, (({}, "realnd "),), lambda c, rng: [gauss(rng, c.batch, *shape)], forward,
        lambda c, ins: np.fft.rfftn(ins[0].astype(np.float64), axes=axes), realnd_tol)
    add(f"irfftn {list(shape)}", 1, make, (({}, "realnd "),),
        lambda c, rng: [np.fft.rfftn(gauss(rng, c.batch, *shape), axes=axes) / math.sqrt(np.prod(shape))], inverse,
        lambda c, ins: np.fft.irfftn(ins[0].astype(np.complex128), s=shape, axes=axes), realnd_tol)


rfftn((16, 64))


def axis(outer, n, inner):
    def make(api, real):
        return ctx_of(api.fa.Fft(n, real, api.device))

    def outer_of(c):
        """the outer count is this case's batch: `outer` at the table's batch, in proportion elsewhere"""
        return outer * c.batch // BATCH

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.transform_axis_ptr(api.ptr(x), out, outer_of(c), inner, FFT), ins[0].shape, ins[0].dtype)

    add(f"axis [{outer}, {n}, {inner}]", 1, make, (({}, "axis "),), lambda c, rng: [cgauss(rng, outer_of(c), n, inner)], run,
        lambda c, ins: np.fft.fft(ins[0].astype(np.complex128), axis=1), axis_tol, describe=lambda c: c.plan.describe_axis(inner))


axis(8, 64, 6)


def r2r(n, kind):
    def make(api, real):
        return ctx_of(api.fa.R2R(n, real, api.device), idx=r2r_truth.want(kind, "ortho", np.zeros((1, n)))[0], norm="ortho")

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.transform_batch_ptr(api.ptr(x), out, c.batch, r2r_truth.KINDS[kind], r2r_truth.NORMS[c.norm]),
                       (c.batch, n), ins[0].dtype)

    add(f"r2r {n} {kind} ortho", 1, make, (({}, "r2r "),), lambda c, rng: [gauss(rng, c.batch, n)], run,
        lambda c, ins: r2r_truth.want(kind, c.norm, ins[0])[1], TWO, pick=lambda c, out: out[:, c.idx])


for _n in (1000, 255):
    for _kind in r2r_truth.KINDS:
        r2r(_n, _kind)


# ---- circular and linear convolution: the amplitude in the signal, and in the filter through set_filters
FILTERS, TAPS = 2, 33


def conv_want(x, h, correlate=False):
    """numpy in f64; row b with filter b mod F (tests/test_gpu_conv.py's want); correlate: with the conjugated spectrum of the taps"""
    n = x.shape[-1]
    hb = h[np.arange(x.shape[0]) % h.shape[0]]
    conj = np.conj if correlate else (lambda v: v)
    if np.iscomplexobj(x):
        return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * conj(np.fft.fft(hb.astype(np.complex128), n, axis=-1)), axis=-1)
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * conj(np.fft.rfft(hb.astype(np.float64), n, axis=-1)), n=n, axis=-1)


def fftconv(n, real_data):
    g = gauss if real_data else cgauss
    kind = "real" if real_data else "complex"

    def make(api, real):
        return ctx_of(api.fa.FftConv(n, real, real_data, api.device), filters=FILTERS, taps=TAPS, correlate=False)

    def run(api, c, ins):
        x, h = api.put(ins[0]), api.put(ins[1])
        c.plan.set_filters_ptr(api.ptr(h), c.taps, c.filters, c.correlate)
        return api.run(lambda out: c.plan.apply_ptr(api.ptr(x), out, c.batch), ins[0].shape, ins[0].dtype)

    if real_data:
        routes = (({"fusion": 1}, "conv real fused untangle: "), ({"fusion": 0}, "conv real composed: "))
    else:
        routes = (({"fusion": 1}, "conv one-launch: "), ({"fusion": 0}, "conv composed: ")) if n == 4096 else (({"fusion": 1}, "conv composed: "),)
    for what, scaled in (("signal", (0,)), ("filter", (1,))):
        add(f"fftconv {n} {kind} scaled {what}", 1, make, routes, lambda c, rng: [g(rng, c.batch, n), g(rng, c.filters, c.taps)], run,
            lambda c, ins: conv_want(ins[0], ins[1], c.correlate), THREE, scaled=scaled)


for _n in (4096, 1000):
    for _real_data in (False, True):
        fftconv(_n, _real_data)


def lconv(lx, k, real_data):
    g = gauss if real_data else cgauss
    off = (k - 1) // 2  # mode "same"

    def make(api, real):
        return ctx_of(api.fa.LinearConv(lx, k, real, "same", real_data, api.device), filters=FILTERS, correlate=False)

    def run(api, c, ins):
        x, h = api.put(ins[0]), api.put(ins[1])
        c.plan.set_filters_ptr(api.ptr(h), c.filters, c.correlate)
        return api.run(lambda out: c.plan.apply_ptr(api.ptr(x), out, c.batch), (c.batch, c.plan.out_length()), ins[0].dtype)

    def truth(c, ins):
        wide = np.float64 if real_data else np.complex128
        taps = np.conj(ins[1][:, ::-1]) if c.correlate else ins[1]  # (correlate: set_filters stores conj(h[K - 1 - i]) in place of h[i])
        return np.array([np.convolve(ins[0][b].astype(wide), taps[b % c.filters].astype(wide))[off:off + lx] for b in range(c.batch)])

    for what, scaled in (("signal", (0,)), ("filter", (1,))):
        add(f"lconv {lx} K={k} same {'real' if real_data else 'complex'} scaled {what}", 1, make, (({}, "lconv overlap-save: "),),
            lambda c, rng: [g(rng, c.batch, lx), g(rng, c.filters, k)], run, truth, THREE, scaled=scaled)


for _real_data in (False, True):
    lconv(3000, 129, _real_data)


# ---- the frame handles
def has_fused_frames(n_fft):
    """the fused frame kernels exist at n_fft 128 ... 1024 in both precisions"""
    return n_fft in (128, 256, 512, 1024)


def frame_ctx(api, cls, real, n_fft, hop, *more):
    plan = cls(n_fft, *more, real, hop, None, True, "reflect", api.device)
    w = window(np.random.default_rng(n_fft + hop), real, n_fft)
    dw = api.put(w)
    plan.set_window_ptr(api.ptr(dw))
    return ctx_of(plan, w=w, dw=dw)


def frames_of(n_fft):
    """67 frames a row at n_fft 256: the fused tiles (64 frames at f32, 32 at f64; frame pairs: half as many) are more than one a row,
    the last partly empty; 35 at 400: two slots of the composed sums"""
    return 67 if n_fft == 256 else 35


def stft(n_fft, hop):
    nf = frames_of(n_fft)
    length, bins = (nf - 1) * hop + 3, n_fft // 2 + 1
    fused = has_fused_frames(n_fft)

    def make(api, real):
        c = frame_ctx(api, api.fa.Stft, real, n_fft, hop)
        assert c.plan.frames(length) == stft_truth.frames(length, n_fft, hop, "reflect") == nf
        return restate(c, length, nf)

    def forward(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.length, c.batch, c.normalized), (c.batch, c.nf, bins), cdt(c.plan.real))

    def inverse(api, c, ins):
        s = api.put(ins[0])
        back = c.plan.default_length(c.nf)
        return api.run(lambda out: c.plan.inverse_ptr(api.ptr(s), out, c.nf, back, c.batch, c.normalized), (c.batch, back), rdt(c.plan.real))

    add(f"stft {n_fft} hop {hop}", 1, make, fusion_routes("stft fused rows, istft composed: real ", "stft composed, istft composed: real ", lambda real: fused),
        lambda c, rng: [gauss(rng, c.batch, c.length)], forward, lambda c, ins: stft_truth.stft(ins[0], n_fft, hop, n_fft, c.w, "reflect", c.normalized), TWO)
    add(f"istft {n_fft} hop {hop}", 1, make, (({"fusion": 0}, "stft composed, istft composed: real "),),
        lambda c, rng: [half_spectrum(rng, (c.batch, c.nf), n_fft)], inverse,
        lambda c, ins: stft_truth.istft(ins[0], n_fft, hop, c.plan.default_length(c.nf), n_fft, c.w, "reflect", c.normalized), FOUR)


stft(256, 64)
stft(400, 160)


def mdct(n):
    length = 9 * n + 5
    fused = "mdct fused rows, imdct composed: " if n % 2 == 0 else None
    composed = "mdct composed, imdct composed: " if n % 2 == 0 else "mdct full-length, imdct full-length: "

    def make(api, real):
        plan = api.fa.Mdct(n, real, True, api.device)
        w = window(np.random.default_rng(n), real, 2 * n)
        dw = api.put(w)
        plan.set_window_ptr(api.ptr(dw))
        nf = plan.frames(length)
        assert nf == mdct_truth.frames(length, n, True) == 11
        return ctx_of(plan, w=w, dw=dw, nf=nf, length=length)

    def forward(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.length, c.batch, c.normalized), (c.batch, c.nf, n), ins[0].dtype)

    def inverse(api, c, ins):
        s = api.put(ins[0])
        return api.run(lambda out: c.plan.inverse_ptr(api.ptr(s), out, c.nf, c.length, c.batch, c.normalized), (c.batch, c.length), ins[0].dtype)

    add(f"mdct {n}", 1, make, fusion_routes(fused, composed, lambda real: fused is not None), lambda c, rng: [gauss(rng, c.batch, c.length)], forward,
        lambda c, ins: mdct_truth.mdct(ins[0], n, c.w, True, c.normalized), TWO)
    add(f"imdct {n}", 1, make, (({"fusion": 0}, composed),), lambda c, rng: [gauss(rng, c.batch, c.nf, n)], inverse,
        lambda c, ins: mdct_truth.imdct(ins[0], n, c.length, c.w, True, c.normalized), FOUR)


mdct(256)
mdct(255)


def pfb(P, T, D, real_rows):
    nf = 20
    length = P * T + (nf - 1) * D
    bins = P // 2 + 1 if real_rows else P
    kind = "real" if real_rows else "complex"

    def make_with(cls):
        def make(api, real):
            plan = cls(api.fa)(P, T, real, D, real_rows, api.device)
            h = np.ascontiguousarray(np.random.default_rng(P + T).standard_normal(P * T).astype(rdt(real)))
            dh = api.put(h)
            plan.set_filter_ptr(api.ptr(dh))
            return ctx_of(plan, h=h, dh=dh, length=length, nf=nf)
        return make

    def forward(api, c, ins):
        assert c.plan.frames(c.length) == pfb_truth.frames(c.length, P, T, D) == c.nf
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.length, c.batch), (c.batch, c.nf, bins), cdt(c.plan.real))

    def inverse(api, c, ins):
        assert c.plan.length(c.nf) == ipfb_truth.full(c.nf, P, T, D) == c.length
        s = api.put(ins[0])
        return api.run(lambda out: c.plan.inverse_ptr(api.ptr(s), out, c.nf, c.length, c.batch), (c.batch, c.length),
                       rdt(c.plan.real) if real_rows else cdt(c.plan.real))

    add(f"pfb P={P} T={T} D={D} {kind}", 1, make_with(lambda fa: fa.Pfb), fusion_routes("pfb fused rows: ", "pfb composed: "),
        lambda c, rng: [(gauss if real_rows else cgauss)(rng, c.batch, c.length)], forward,
        lambda c, ins: pfb_truth.pfb(ins[0], c.h, P, T, D, real_rows), TWO)
    add(f"ipfb P={P} T={T} D={D} {kind}", 1, make_with(lambda fa: fa.Ipfb), (({}, "ipfb composed: "),),
        lambda c, rng: [half_spectrum(rng, (c.batch, c.nf), P) if real_rows else cgauss(rng, c.batch, c.nf, P)], inverse,
        lambda c, ins: ipfb_truth.synth(ins[0], c.h, P, T, D, real_rows, c.length), TWO)


pfb(256, 4, 192, True)
pfb(256, 4, 192, False)


def resample(n, m, complex_rows):
    def make(api, real):
        plan = api.fa.Resample(n, m, real, api.device, not complex_rows)
        w = resample_truth.window(np.random.default_rng(n + m), n, rdt(real))
        dw = api.put(w)
        plan.set_window_ptr(api.ptr(dw))
        return ctx_of(plan, w=w, dw=dw)

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.batch), (c.batch, m), ins[0].dtype)

    routes = (({"fusion": 0}, "resample complex: "),) if complex_rows else fusion_routes("resample real fused untangle: ", "resample real composed: ")
    add(f"resample {n} -> {m} {'complex' if complex_rows else 'real'}", 1, make, routes,
        lambda c, rng: [(cgauss if complex_rows else gauss)(rng, c.batch, n)], run, lambda c, ins: resample_truth.resample(ins[0], m, c.w), TWO)


resample(3000, 2756, False)
resample(1000, 1031, True)


def czt(n, m, real_input):
    def make(api, real):
        return ctx_of(api.fa.Czt(n, m, 1.0, None, 1.0, 0.0, real, real_input, api.device))

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.transform_ptr(api.ptr(x), out, c.batch), (c.batch, m), cdt(c.plan.real))

    add(f"czt {n} -> {m} {'real' if real_input else 'complex'}", 1, make, fusion_routes("czt one-launch: ", "czt composed: "),
        lambda c, rng: [(gauss if real_input else cgauss)(rng, c.batch, n)], run, lambda c, ins: czt_truth.czt(ins[0], m, 1.0, -1.0 / m), czt_tol)


czt(1000, 1000, False)
czt(1000, 1000, True)


def hilbert(n):
    def make(api, real):
        return ctx_of(api.fa.Hilbert(n, real, api.device))

    def analytic(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.analytic_ptr(api.ptr(x), out, c.batch), (c.batch, n), cdt(c.plan.real))

    def envelope(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.envelope_ptr(api.ptr(x), out, c.batch), (c.batch, n), ins[0].dtype)

    routes = fusion_routes("hilbert one-launch: ", "hilbert composed: ", lambda real: n == 2048)
    add(f"hilbert analytic {n}", 1, make, routes, lambda c, rng: [gauss(rng, c.batch, n)], analytic, lambda c, ins: hilbert_truth.analytic(ins[0]), TWO)
    add(f"hilbert envelope {n}", 1, make, routes, lambda c, rng: [gauss(rng, c.batch, n)], envelope, lambda c, ins: hilbert_truth.envelope(ins[0]), TWO,
        integers=n == 2048, edge=True)


hilbert(2048)
hilbert(1000)


# ---- power, magnitude, Welch; cross spectrum and coherence; band energies
def spectrogram(n_fft, hop):
    nf = frames_of(n_fft)
    length, bins = (nf - 1) * hop + 3, n_fft // 2 + 1
    routes = fusion_routes("spectrogram fused rows, welch fused rows: real ", "spectrogram composed, welch composed: real ",
                           lambda real: has_fused_frames(n_fft))

    def make(api, real):
        c = frame_ctx(api, api.fa.Spectrogram, real, n_fft, hop)
        assert c.plan.frames(length) == nf
        return restate(c, length, nf)

    def forward(power):
        def run(api, c, ins):
            x = api.put(ins[0])
            return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.length, c.batch, power, power == 1), (c.batch, c.nf, bins), ins[0].dtype)
        return run

    def welch(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.welch_ptr(api.ptr(x), out, c.length, c.batch, c.fold, c.scale), (c.batch, bins), ins[0].dtype)

    for power in (2, 1):
        add(f"spectrogram {n_fft} hop {hop} power {power}", power, make, routes, lambda c, rng: [gauss(rng, c.batch, c.length)], forward(power),
            lambda c, ins, power=power: spectrogram_truth.spectrogram(ins[0], n_fft, hop, n_fft, c.w, "reflect", power, power == 1), FOUR,
            integers=n_fft == 256, edge=power == 1)
    add(f"welch {n_fft} hop {hop}", 2, make, routes, lambda c, rng: [gauss(rng, c.batch, c.length)], welch,
        lambda c, ins: spectrogram_truth.welch(ins[0], n_fft, hop, n_fft, c.w, "reflect", c.fold, c.scale), FOUR, integers=n_fft == 256)


spectrogram(256, 64)
spectrogram(400, 160)


def cross_spectrum(n_fft, hop):
    nf = frames_of(n_fft)
    length, bins = (nf - 1) * hop + 3, n_fft // 2 + 1
    routes = fusion_routes("csd fused rows, coherence fused rows: real ", "csd composed, coherence composed: real ",
                           lambda real: has_fused_frames(n_fft))

    def make(api, real):
        c = frame_ctx(api, api.fa.CrossSpectrum, real, n_fft, hop)
        assert c.plan.frames(length) == nf
        return restate(c, length, nf)

    def inputs(c, rng):
        return list(csd_truth.pair(rng, c.batch, c.length, np.float64))

    def csd(api, c, ins):
        x, y = api.put(ins[0]), api.put(ins[1])
        return api.run(lambda out: c.plan.csd_ptr(api.ptr(x), api.ptr(y), out, c.length, c.batch, c.fold, c.scale), (c.batch, bins), cdt(c.plan.real))

    def coherence(api, c, ins):
        x, y = api.put(ins[0]), api.put(ins[1])
        return api.run(lambda out: c.plan.coherence_ptr(api.ptr(x), api.ptr(y), out, c.length, c.batch), (c.batch, bins), ins[0].dtype)

    add(f"csd {n_fft} hop {hop}", 2, make, routes, inputs, csd,
        lambda c, ins: csd_truth.csd(ins[0], ins[1], n_fft, hop, n_fft, c.w, "reflect", c.fold, c.scale), csd_tol, integers=n_fft == 256)
    add(f"coherence {n_fft} hop {hop}", 0, make, routes, inputs, coherence,
        lambda c, ins: csd_truth.coherence(ins[0], ins[1], n_fft, hop, n_fft, c.w, "reflect"), coherence_tol, integers=n_fft == 256)


cross_spectrum(256, 64)
cross_spectrum(400, 160)


def band_spectrogram(n_fft, hop, bands):
    nf = frames_of(n_fft)
    length = (nf - 1) * hop + 3

    def make(api, real):
        c = frame_ctx(api, api.fa.BandSpectrogram, real, n_fft, hop, bands)
        W = api.fa.mel_filterbank(n_fft // 2 + 1, 0.0, 8000.0, bands, 16000.0, None, "htk")
        c.W = np.asarray(W).astype(rdt(real)).astype(np.float64)  # what the handle holds: the truth uses the rounded weights
        c.plan.set_bands(c.W)
        assert c.plan.frames(length) == nf and c.plan.bands() == bands
        c.held_floor = None
        return restate(c, length, nf)

    def want(c, ins, power):
        return bandspec_truth.band_spectrogram(ins[0], c.W, n_fft, hop, n_fft, c.w, "reflect", power, power == 1)

    def forward(power, log):
        def run(api, c, ins):
            # under the log the floor is the median of the truth at this input: about half of the values clamp
            c.floor = (float(np.median(want(c, ins, power))) if c.held_floor is None else c.held_floor) if log else 0.0
            x = api.put(ins[0])
            return api.run(lambda out: c.plan.forward_ptr(api.ptr(x), out, c.length, c.batch, power, power == 1, LOG_MULT if log else 0.0, c.floor),
                           (c.batch, c.nf, bands), ins[0].dtype)
        return run

    routes = fusion_routes("bandspec fused rows: real ", "bandspec composed: real ")
    for power in (1, 2):
        add(f"bandspec {n_fft} {bands} bands power {power}", power, make, routes, lambda c, rng: [gauss(rng, c.batch, c.length)], forward(power, False),
            lambda c, ins, power=power: want(c, ins, power), FOUR)
        add(f"bandspec {n_fft} {bands} bands power {power} log", None, make, routes, lambda c, rng: [gauss(rng, c.batch, c.length)], forward(power, True),
            lambda c, ins, power=power: np.maximum(want(c, ins, power), c.floor), FOUR, kd=power,
            err=lambda c, out, w: rel_l2(np.exp(out.astype(np.float64) / LOG_MULT), w), integers=power == 2,
            hold=lambda c, ins, power=power: setattr(c, "held_floor", float(np.median(want(c, ins, power)))))


band_spectrogram(256, 64, 20)


# ---- the five newer handles.  One proxy serves the families whose cases are several handles at once (two lag windows, two accuracies):
# set_option goes to every handle, or, for the key `pick`, chooses the one that describe() speaks for
class Plans:
    def __init__(self, plans, pick=None):
        self.plans, self.pick, self.now = list(plans), pick, 0

    def set_option(self, key, value):
        if key == self.pick:
            self.now = value
            return
        for p in self.plans:
            p.set_option(key, value)

    def describe(self):
        return self.plans[self.now].describe()

    @property
    def plan(self):
        return self.plans[self.now]


# cross-correlation and GCC-PHAT: both lag windows of a shape in one case, the short one and the whole row (the direct store)
def xcorr_windows(L):
    return ((-5, 11), (0, L))


def xcorr_has_kernel(real, L, phat):
    """the product's one-launch table, tests/test_gpu_xcorr.py's has_kernel without the development switch"""
    return L in (2048, 4096, 8192, 16384) and real == "f64" and not phat


def xcorr(L, n, cplx, composed_only=False):
    kind = "complex" if cplx else "real"
    wins = xcorr_windows(L)

    def make(api, real):
        return ctx_of(Plans([api.fa.CrossCorrelation(n, L, first, lags, real, not cplx, api.device) for first, lags in wins]))

    def routes_of(phat):
        def routes(real):
            fused = not cplx and not composed_only and xcorr_has_kernel(real, L, phat)
            both = (({"weighting": phat, "fusion": 1}, "xcorr one-launch: "), ({"weighting": phat, "fusion": 0}, "xcorr composed: "))
            return both if fused else (({"weighting": phat, "fusion": 1}, "xcorr composed: "),)
        return routes

    def run(api, c, ins):
        x, y = api.put(ins[0]), api.put(ins[1])
        dt = ins[0].dtype
        return np.concatenate([api.run(lambda out: p.correlate_ptr(api.ptr(x), api.ptr(y), out, c.batch), (c.batch * p.lags(),), dt) for p in c.plan.plans])

    def truth_of(phat):
        return lambda c, ins: xcorr_truth.full(ins[0], ins[1], L, bool(phat))

    def err(c, out, want):
        """tests/test_gpu_xcorr.py's measure, the worse of the two windows"""
        worst, at = 0.0, 0
        for first, lags in wins:
            worst = max(worst, xcorr_truth.window_err(out[at:at + c.batch * lags].reshape(c.batch, lags), want, first, lags))
            at += c.batch * lags
        return worst

    g = cgauss if cplx else gauss
    white = lambda c, rng: [g(rng, c.batch, n), g(rng, c.batch, n)]  # noqa: E731
    opposite = dict(signs={1: -1}, ks=lambda real: OPPOSITE[real])
    where = f"{L} n={n} {kind}" + (" composed" if composed_only else "")
    add(f"xcorr {where} scaled x", 1, make, routes_of(0), white, run, truth_of(0), THREE, scaled=(0,), err=err, integers=True)
    add(f"xcorr {where} scaled x and y", 2, make, routes_of(0), white, run, truth_of(0), THREE, err=err, integers=True)
    add(f"xcorr {where} opposite", 0, make, routes_of(0), white, run, truth_of(0), THREE, err=err, **opposite)

    # PHAT: the spike rows of the family's tests and their bound, base x (sqrt(2 (kx^2 + ky^2)) + 1) under kx, ky <= 3
    def spikes(c, rng):
        return list(xcorr_truth.spike_rows(rng, c.batch, n, 2, np.complex128 if cplx else np.float64))

    def conditions(c, ins):
        c.kx, c.ky = xcorr_truth.kappa(ins[0], L), xcorr_truth.kappa(ins[1], L)
        assert c.kx <= 3 and c.ky <= 3, (c.kx, c.ky)

    def bound(c, d, real):
        return base_tol(d, real) * (math.sqrt(2 * (c.kx * c.kx + c.ky * c.ky)) + 1)

    def largest_bin(c, ins, y0):
        wide = np.complex128 if cplx else np.float64
        return float(max(np.abs(np.fft.fft(a.astype(wide), L, axis=-1)).max() for a in ins))

    phat = dict(err=err, conditions=conditions, bound=bound)
    add(f"gcc-phat {where} scaled x and y", 0, make, routes_of(1), spikes, run, truth_of(1), None, edge=True, edge_of=largest_bin, **phat)
    add(f"gcc-phat {where} opposite", 0, make, routes_of(1), spikes, run, truth_of(1), None, **phat, **opposite)


xcorr(2048, 1501, False)
xcorr(1000, 600, False)
xcorr(255, 100, True)


# fractional delay and delay-and-sum: three groups of C rows; the amplitude in the rows, or in the weights; never in the delays
def delay(L, n, cplx, channels):
    def rows_of(c):
        return c.batch * channels

    def make(api, real):
        return ctx_of(api.fa.Delay(n, L, real, not cplx, channels, api.device))

    def inputs(c, rng):
        rows = rows_of(c)
        delays = np.array((delay_truth.DELAYS * -(-rows // len(delay_truth.DELAYS)))[:rows])
        return [(cgauss if cplx else gauss)(rng, rows, n), delays, rng.uniform(0.5, 2.0, rows)]

    def run(api, c, ins):
        x, d, w = (api.put(a) for a in ins)
        return api.run(lambda out: c.plan.apply_ptr(api.ptr(x), api.ptr(d), api.ptr(w), out, rows_of(c)), (c.batch, n), ins[0].dtype)

    def truth(c, ins):
        c.ins = ins
        return delay_truth.delay(ins[0], ins[1], L, channels, ins[2])

    def err(c, out, want):
        return delay_truth.err(out, want, c.ins[0], channels, c.ins[2])

    fused = not cplx and channels == 1 and delay_cases.has_kernel("f64", L) and delay_cases.has_kernel("f32", L)
    routes = fusion_routes("delay one-launch: ", "delay composed: ", lambda real: fused)
    where = f"{L} n={n} {'complex' if cplx else 'real'} C={channels}"
    add(f"delay {where} scaled input", 1, make, routes, inputs, run, truth, THREE, scaled=(0,), err=err, integers=True)
    add(f"delay {where} scaled weights", 1, make, routes, inputs, run, truth, THREE, scaled=(2,), err=err)


delay(2048, 1501, False, 1)
delay(1000, 600, False, 1)
delay(1000, 600, False, 3)
delay(255, 100, True, 1)


# N-D convolution: a bank of 2 filters, `correlate` off and on in one case; the amplitude in the items, or in the taps (set again at
# every k)
def convnd(shape):
    taps = tuple(min(3, n) for n in shape)

    def make(api, real):
        return ctx_of(api.fa.FftConvNd(shape, real, api.device), where="emu" if api.device < 0 else "gpu", filters=FILTERS, window=None, filter_first=0)

    def run(api, c, ins):
        x, h = api.put(ins[0]), api.put(ins[1])
        if c.window is not None:  # (in_shape, out_first, out_shape), stated by the caller; None: the handle as created
            c.plan.set_window(*c.window)
        outs = []
        for correlate in (False, True):
            c.plan.set_filters_ptr(api.ptr(h), taps, c.filters, correlate)
            outs.append(api.run(lambda out: c.plan.apply_ptr(api.ptr(x), out, c.batch, c.filter_first), (c.batch,) + window_of(c)[2], ins[0].dtype))
        return np.stack(outs)

    def window_of(c):
        return c.window if c.window is not None else (shape, (0,) * len(shape), shape)

    def truth(c, ins):
        _, first, size = window_of(c)
        return np.stack([convnd_truth.window(convnd_truth.circular(ins[0], ins[1], shape, correlate, c.filter_first), first, size)
                         for correlate in (False, True)])

    def bound(c, d, real):
        return convnd_cases.bound(c, c.plan, real)

    routes = fusion_routes("convnd fused untangle: ", "convnd composed: ", lambda real: convnd_cases.has_fused(shape))
    for what, scaled in (("items", (0,)), ("taps", (1,))):
        add(f"convnd {list(shape)} scaled {what}", 1, make, routes, lambda c, rng: [gauss(rng, c.batch, *window_of(c)[0]), gauss(rng, c.filters, *taps)], run, truth,
            None, scaled=scaled, bound=bound, integers=what == "items")


for _shape in ((4, 6), (4, 7), (3, 4, 10), (3, 5, 9)):
    convnd(_shape)


# non-uniform FFT: both signs and both mode orders in one case; the amplitude in the strengths (type 1) or the modes (type 2); never in
# the points.  The figure is err / bound with tests/nufft_cases.py's bound of each call, 3 x 10^(1 - w) plus its rounding term, held
# against 1; terms() asserts the condition on the inputs (the f64 model within 2.5 x 10^(1 - w) of the direct sum) first.
NUFFT_EPS = {"f32": (1e-6,), "f64": (1e-6, 1e-12)}
NUFFT_CALLS = tuple((sign, order) for sign in (-1, 1) for order in (0, 1))


def nufft(n, point_set):
    def make(api, real):
        c = ctx_of(Plans([api.fa.Nufft(n, eps, real, api.device) for eps in NUFFT_EPS[real]], pick="accuracy"), real=real, xs=[])
        for plan, eps in zip(c.plan.plans, NUFFT_EPS[real]):
            c.xs.append(nufft_cases.points(point_set, n, eps, real))
            plan.set_points(c.xs[-1])
        return c

    def routes(real):
        out = []
        for i, eps in enumerate(NUFFT_EPS[real]):
            w = nufft_truth.width(eps, real)
            for table in (0, 1):
                out.append(({"accuracy": i, "table": table}, f"nufft {nufft_cases.ROUTES[table]}: w {w}, L {nufft_truth.grid_length(n, w)}, "))
        return tuple(out)

    def run_of(typ):
        def run(api, c, ins):
            plan = c.plan.plan
            v = api.put(ins[0])
            call = plan.to_modes_ptr if typ == 1 else plan.to_points_ptr
            shape = (c.batch, plan.modes() if typ == 1 else plan.points())
            return np.stack([api.run(lambda out: call(api.ptr(v), out, c.batch, sign, order), shape, ins[0].dtype) for sign, order in NUFFT_CALLS])
        return run

    def truth_of(typ):
        def truth(c, ins):
            c.v, x = ins[0], c.xs[c.plan.now]
            return np.stack([nufft_cases.want_of(typ, x, ins[0], n, sign, order) for sign, order in NUFFT_CALLS])
        return truth

    def err_of(typ):
        def err(c, out, want):
            eps, x = NUFFT_EPS[c.real][c.plan.now], c.xs[c.plan.now]
            return max(rel_l2(out[i], want[i]) / nufft_cases.bound(c.real, n, eps, x, typ, c.v, sign, order, want[i])
                       for i, (sign, order) in enumerate(NUFFT_CALLS))
        return err

    one = lambda d, real: 1.0  # noqa: E731
    add(f"nufft type 1 N={n} {point_set} scaled strengths", 1, make, routes, lambda c, rng: [cgauss(rng, c.batch, c.plan.plan.points())], run_of(1), truth_of(1), one,
        err=err_of(1), integers=True)
    add(f"nufft type 2 N={n} {point_set} scaled modes", 1, make, routes, lambda c, rng: [cgauss(rng, c.batch, n)], run_of(2), truth_of(2), one,
        err=err_of(2), integers=True)


for _n, _set in ((100, "random37"), (101, "random37"), (101, "last_cell")):
    assert _n in nufft_cases.sizes_for(_set)
    nufft(_n, _set)


# cepstrum and minimum phase: no exact scaling (the logarithm), so (b) at k = +-40 / +-300 in the family's own measure, which divides by
# kappa and does not change with scale, and the identity between the two results that the truths satisfy exactly:
#   cepstrum       c(2^k x) = c(x) + k log_mult ln 2 at quefrency 0          minimum phase   h(2^k x) = 2^(k log_mult) h(x)
def cepstrum(L, n, mode, log_mult):
    def make(api, real):
        return ctx_of(api.fa.Cepstrum(n, L, real, n, mode, api.device))

    def conditions(c, ins):
        """tests/cepstrum_cases.py's conditions (both scale-invariant), without its line of output"""
        kappa, phase = float(cepstrum_truth.kappa(ins[0], L).max()), cepstrum_truth.max_phase(ins[0], L, log_mult)
        assert kappa <= 4 and phase <= np.pi, (L, n, kappa, phase)

    def run(api, c, ins):
        x = api.put(ins[0])
        return api.run(lambda out: c.plan.apply_ptr(api.ptr(x), out, c.batch, log_mult, 0.0), (c.batch, n), ins[0].dtype)

    def truth(c, ins):
        c.x = ins[0]
        return cepstrum_truth.full(mode, ins[0], L, log_mult)[:, :n]

    def err(c, out, want):
        return cepstrum_truth.err(mode, out, c.x, L, n, log_mult)

    def bound(c, d, real):
        return (3 if mode == cepstrum_truth.CEPSTRUM else 6) * base_tol(d, real)

    def identity(c, k, s, o, ins):
        s, o = s.astype(np.float64), o.astype(np.float64)
        den = abs(log_mult) * cepstrum_truth.kappa(ins[0], L)
        if mode == cepstrum_truth.CEPSTRUM:
            s[:, 0] -= k * log_mult * math.log(2.0)
        else:
            s = np.ldexp(s, -k * int(log_mult))
            den = den * np.linalg.norm(cepstrum_truth.full(mode, ins[0], L, log_mult), axis=-1)
        return float(np.max(np.linalg.norm(s - o, axis=-1) / den))

    def largest_bin(c, ins, y0):
        return float(np.abs(cepstrum_truth.spectrum(ins[0], L)).max())

    fused = all(cepstrum_cases.has_kernel(real, mode, L) for real in ("f32", "f64"))
    name = cepstrum_cases.MODE_NAME[mode]
    routes = fusion_routes(f"cepstrum one-launch ({name}): ", f"cepstrum composed ({name}): ", lambda real: fused)
    samples = mode == cepstrum_truth.CEPSTRUM  # the minimum-phase input is a filter, not samples
    add(f"cepstrum {L} n={n} {name} log_mult {log_mult:+d}", None, make, routes, lambda c, rng: [cepstrum_truth.rows(rng, c.batch, n, np.float64)], run, truth,
        None, kd=1, err=err, bound=bound, conditions=conditions, identity=identity, integers=samples, edge=samples, edge_of=largest_bin)


for _L, _n in ((2048, 1501), (1000, 600)):
    for _mode in cepstrum_cases.MODES:
        for _log_mult in (1, -1):
            cepstrum(_L, _n, _mode, _log_mult)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = list(BY_NAME)
INTEGER_NAMES = [c.name for c in CASES if c.integers]
EDGE_NAMES = [c.name for c in CASES if c.edge]
