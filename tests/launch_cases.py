"""The handles' launch splits at small shapes: the cases and their assertions, stated once and run twice -- on the CPU emulation
(tests/test_launch_emu.py) and on the MI355X through the experiments library (tests/test_gpu_launch.py).  A handle cuts what it hands
to one kernel launch so that the kernel's 32-bit indices and 31-bit byte offsets stay in range: at most REAL_LAUNCH_BYTES = 2^31 - 1
bytes of either side of a sweep, at most 2^30 frames, rows, lanes or workgroups of a launch.  Under the product's 1 GiB scratch bound a
chunk is smaller than a launch, so those loops take one turn.  The experiments library and the emulator build read the two bounds from
the environment at create (launch_bound, handle_common.h):
  FOURIER_LAUNCH_BYTES   what the rows_per of every REAL_LAUNCH_BYTES split divides
  FOURIER_LAUNCH_ITEMS   LAUNCH_ITEMS (frames; samples and lanes of the synthesis bank's gather), LAUNCH_WORKGROUPS (the linear
                         convolution) and the 2^30-row walks of the one-launch routes
which brings every split down to batches of 3 to 7.  The callers hand in an adapter (`api`): it creates handles under switches, uploads
numpy arrays, hands out their addresses and runs an entry point into an output between guard elements, prefilled with NaN.

How a call is cut is restated from the plans so that every case asserts that it takes more than one launch and where the cuts fall:
  a byte sweep over the nb rows of a chunk    rows_per = max(1, bound // row), row the larger side's bytes per row as the plan's sweep()
                                              states it; launches of rows_per rows, fewer in the last; a bound below one row: one row
  the chunks of a call                        max(1, min(batch, scratch bound // scratch bytes per row)) rows (chunk_rows)
  a fused frame route                         launches of `items` frames of the flat frame index batch x frames
  Welch / cross-spectrum row groups           min(rows the partials' bound holds, max(1, items // max(frames, tiles x 32))) rows
  the synthesis bank's gather                 pieces of `items` samples of a range, each in launches of max(1, items // samples) rows
  overlap-save / the padded route's copies    launches of max(1, items // workgroups per row) rows

Comparisons.  Against a handle of the same library created without the bound, on the same buffers: bit for bit, everywhere.  A launch
split moves no arithmetic -- every output element is computed by the same lane expression from the same inputs -- and the cases whose
sums could re-associate (the composed Welch average and cross spectrum, tests/chunk_walks.py) are given bounds under which every launch
ends on a slot of partials.  Against the f64 truth modules: the tolerance of the handle's own GPU test, restated beside each case.
Every figure is printed with its bound before it is asserted; the inputs are compared with what was uploaded afterwards."""
import numpy as np

import bandspec_truth
import csd_truth
import czt_truth
import hilbert_truth
import ipfb_truth
import mdct_truth
import pfb_truth
import r2r_truth
import resample_truth
import spectrogram_truth
import stft_truth
import xcorr_truth
from helpers import rel_l2

BYTES = "FOURIER_LAUNCH_BYTES"
ITEMS = "FOURIER_LAUNCH_ITEMS"
REAL = "FOURIER_REAL_SCRATCH_BYTES"
CONV = "FOURIER_CONV_SCRATCH_BYTES"
FUSED_TILE = {"f32": 64, "f64": 32}  # frames per workgroup of the fused frame kernels at n_fft = 256 (tests/chunk_walks.py)
WELCH_TILE = 32
CSD_PLANES = 4
LCONV_SEG = 2048                     # words per workgroup of lconv_copy_kernel (kernel_args.h)
BATCH = 7
WORST = {}
# (n, m) of the chirp-z sweeps: L = 128 and 256
CZT_SHAPES = ((64, 63), (250, 7))
# (n, m, complex rows, "fusion"): the packed even case, h odd, odd sizes; up and down
RESAMPLE_SHAPES = ((64, 250, True, 0), (250, 63, True, 0), (64, 250, False, 1), (250, 64, False, 1), (64, 250, False, 0), (63, 64, False, 0))
# (n, real data, "fusion")
CONV_SHAPES = ((250, False, 0), (63, False, 0), (64, True, 1), (250, True, 1), (250, True, 0), (63, True, 0))


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def elem(real):
    """bytes of one complex value"""
    return 8 if real == "f32" else 16


def base(describe, real):
    """tests/test_gpu_real.py's tol(): one transform of the inner plan"""
    blu = "bluestein" in describe
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def chunks_of(total, chunk):
    return [(g0, min(chunk, total - g0)) for g0 in range(0, total, chunk)]


def chunk_rows(batch, cap, per):
    return max(1, min(batch, cap // per))


def sizes(total, per):
    return [n for _, n in chunks_of(total, per)]


def byte_walk(batch, bound, row, scratch=None, per=None):
    """the launches of a byte sweep, chunk by chunk: [[rows of a launch, ...] of a chunk, ...]"""
    chunk = batch if scratch is None else chunk_rows(batch, scratch, per)
    return [sizes(nb, max(1, bound // row)) for nb in sizes(batch, chunk)]


def byte_bounds(row, per, scratch_switch):
    """the bounds of a byte sweep over BATCH = 7 rows and the walk each must give: one row per launch; three rows and eight bytes (a
    ragged last launch); eight bytes (below a row: rows_per clamps to 1); two rows under a scratch of four rows (a split inside the
    second chunk)"""
    cases = [("one row", {BYTES: row}, [[1] * 7]), ("ragged", {BYTES: 3 * row + 8}, [[3, 3, 1]]), ("below a row", {BYTES: 8}, [[1] * 7]),
             ("inside the second chunk", {BYTES: 2 * row, scratch_switch: 4 * per}, [[2, 2], [2, 1]])]
    for what, env, want in cases:
        walk = byte_walk(BATCH, env[BYTES], row, env.get(scratch_switch), per)
        assert walk == want and sum(len(c) for c in walk) > 1, (what, walk)
    return [(what, env) for what, env, _ in cases]


def figure(family, real, what, value, bound):
    """print, record, assert"""
    print(f"launch {family} {real} {what}: figure {value:.3g} bound {bound:.3g} ratio {value / bound:.3g}")
    WORST[family, real] = max(WORST.get((family, real), 0.0), value / bound)
    assert value <= bound, (family, real, what, value, bound)


def print_worst():
    for key, v in sorted(WORST.items()):
        print(f"launch splits worst figure / bound {key}: {v:.3g}")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def randn(rng, shape, dtype):
    v = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return np.ascontiguousarray(v.astype(dtype))


def uniform(rng, real, n):
    """window or filter values in [0.5, 1.5]"""
    return np.ascontiguousarray((0.5 + rng.random(n)).astype(rdt(real)))


class HostApi:
    """the adapter of the CPU emulation build: `fa` is fourier_amd bound to it, the buffers are host memory"""
    GUARD = 64
    SENTINEL = 77.0

    def __init__(self, fa, monkeypatch):
        self.fa, self.monkeypatch = fa, monkeypatch

    def create(self, make, **env):
        """make(fa) with the development switches `env` set: they are read at create only"""
        for k, v in env.items():
            self.monkeypatch.setenv(k, str(v))
        try:
            return make(self.fa)
        finally:
            for k in env:
                self.monkeypatch.delenv(k)

    def put(self, a):
        return a.copy()

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf

    def run(self, call, shape, dtype):
        count = int(np.prod(shape))
        buf = np.full(count + 2 * self.GUARD, self.SENTINEL, dtype)
        out = buf[self.GUARD:self.GUARD + count]
        out[:] = np.nan
        call(out.ctypes.data)
        assert np.all(buf[:self.GUARD] == self.SENTINEL) and np.all(buf[-self.GUARD:] == self.SENTINEL), "a guard element was written"
        return out.reshape(shape).copy()


class Call:
    """one entry point of a case: fn(plan, out_ptr) writes `shape` values of `dtype`; err(got) is the figure against the truth and
    bound(describe) what it must stay within"""

    def __init__(self, name, shape, dtype, fn, err, bound):
        self.name, self.shape, self.dtype, self.fn, self.err, self.bound = name, shape, dtype, fn, err, bound


def l2_call(name, want, dtype, fn, factor, real):
    """the usual figure: relative L2 against `want` within factor x base()"""
    return Call(name, want.shape, dtype, fn, lambda got: rel_l2(got, want), lambda d: factor * base(d, real))


def compare(api, real, family, tag, make, prefix, inputs, calls, bounds, always=None):
    """Every call on a handle created without a bound (against the truth), then under each (what, switches) of `bounds`: the same describe
    string, the truth's tolerance, and the unbounded handle's bits.  `inputs`: (host array, device buffer) pairs that must come back
    unchanged.  `always`: switches of both handles (what selects the route)."""
    always = always or {}
    ref = api.create(make, **always)
    d = ref.describe()
    assert d.startswith(prefix), (d, prefix)
    full = {}
    for c in calls:
        full[c.name] = api.run(lambda out, c=c: c.fn(ref, out), c.shape, c.dtype)
        figure(family, real, f"{tag} {c.name} unbounded [{d}]", c.err(full[c.name]), c.bound(d))
    for what, env in bounds:
        small = api.create(make, **dict(always, **env))
        assert small.describe() == d
        for c in calls:
            got = api.run(lambda out, c=c: c.fn(small, out), c.shape, c.dtype)
            figure(family, real, f"{tag} {c.name} {what} {env}", c.err(got), c.bound(d))
            assert same_bits(got, full[c.name]), (family, real, tag, c.name, what, env)
    for host, dev in inputs:
        assert same_bits(np.asarray(api.get(dev)), host), (family, real, tag, "an input was modified")
    return d


# ---- byte sweeps: RealPlan, R2RPlan, HilbertPlan, CztPlan, ResamplePlan, ConvPlan, XcorrPlan
def real_sweep(api, real, n):
    """RealPlan::sweep, even n (an odd n runs grid-stride sweeps over the whole chunk: no split).  row = (h + 1) complex values, the
    half-spectrum side; scratch per row h complex values.  rfft and irfft of 7 rows; tol(): test_gpu_real.py's."""
    assert n % 2 == 0
    rng = np.random.default_rng(11 + n)
    h = n // 2
    xh = randn(rng, (BATCH, n), rdt(real))
    sh = randn(rng, (BATCH, h + 1), cdt(real))
    sh[:, 0] = sh[:, 0].real
    sh[:, -1] = sh[:, -1].real
    x, s = api.put(xh), api.put(sh)
    calls = [l2_call("rfft", np.fft.rfft(xh.astype(np.float64), axis=-1), cdt(real),
                     lambda p, out: p.forward_batch_ptr(api.ptr(x), out, BATCH), 1, real),
             l2_call("irfft", np.fft.irfft(sh.astype(np.complex128), n=n, axis=-1), rdt(real),
                     lambda p, out: p.inverse_batch_ptr(api.ptr(s), out, BATCH), 1, real)]
    compare(api, real, "real", f"n={n}", lambda fa: fa.RealFft(n, real), "real half-length: ", [(xh, x), (sh, s)], calls,
            byte_bounds((h + 1) * elem(real), h * elem(real), REAL))


def r2r_sweep(api, real, n):
    """R2RPlan::sweep, even n.  row = h complex values = N reals (both sides); scratch per row two halves of h complex values.  Every
    kind, backward and ortho; tol(): test_gpu_r2r.py's, twice the base."""
    assert n % 2 == 0
    rng = np.random.default_rng(12 + n)
    h = n // 2
    xh = randn(rng, (BATCH, n), rdt(real))
    x = api.put(xh)
    calls = []
    for kind in r2r_truth.KINDS:
        for norm in ("backward", "ortho"):
            idx, want = r2r_truth.want(kind, norm, xh)
            calls.append(Call(f"{kind} {norm}", (BATCH, n), rdt(real),
                              lambda p, out, kind=kind, norm=norm: p.transform_batch_ptr(api.ptr(x), out, BATCH, r2r_truth.KINDS[kind],
                                                                                         r2r_truth.NORMS[norm]),
                              lambda got, idx=idx, want=want: rel_l2(got[:, idx], want), lambda d: 2 * base(d, real)))
    compare(api, real, "r2r", f"n={n}", lambda fa: fa.R2R(n, real), "r2r half-length: ", [(xh, x)], calls,
            byte_bounds(h * elem(real), 2 * h * elem(real), REAL))


def hilbert_sweep(api, real, n):
    """HilbertPlan::sweep on the composed route ("fusion" = 0), any n: expand (rows of n / 2 + 1 -> rows of n) and abs (rows of n complex
    values -> rows of n reals).  row = n complex values; scratch per row n / 2 + 1 + n complex values.  The inner RealPlan reads the same
    switches and splits its own sweeps.  tol(): test_gpu_hilbert.py's, twice the base."""
    rng = np.random.default_rng(13 + n)
    xh = hilbert_truth.rows(rng, BATCH, n, rdt(real))
    x = api.put(xh)

    def make(fa):
        p = fa.Hilbert(n, real)
        p.set_option("fusion", 0)
        return p
    calls = [l2_call("analytic", hilbert_truth.analytic(xh), cdt(real), lambda p, out: p.analytic_ptr(api.ptr(x), out, BATCH), 2, real),
             l2_call("envelope", hilbert_truth.envelope(xh), rdt(real), lambda p, out: p.envelope_ptr(api.ptr(x), out, BATCH), 2, real)]
    compare(api, real, "hilbert", f"n={n}", make, "hilbert composed: ", [(xh, x)], calls,
            byte_bounds(n * elem(real), (n // 2 + 1 + n) * elem(real), "FOURIER_HILBERT_SCRATCH_BYTES"))


def one_launch_bounds(batch):
    """the 2^30-row walk of a one-launch route over `batch` = 5 rows: one row per launch, and two (a ragged last launch)"""
    assert sizes(batch, 1) == [1] * 5 and sizes(batch, 2) == [2, 2, 1]
    return [("one row", {ITEMS: 1}), ("ragged", {ITEMS: 2})]


def hilbert_one_launch(api, real):
    """HilbertPlan::run, "fusion" = 1 at n = 2048: one workgroup a row, no scratch; the call walks launches of FOURIER_LAUNCH_ITEMS rows
    with the pointer steps c0 * n reals and c0 * orow bytes"""
    n, batch = 2048, 5
    rng = np.random.default_rng(14)
    xh = hilbert_truth.rows(rng, batch, n, rdt(real))
    x = api.put(xh)

    def make(fa):
        p = fa.Hilbert(n, real)
        p.set_option("fusion", 1)
        return p
    calls = [l2_call("analytic", hilbert_truth.analytic(xh), cdt(real), lambda p, out: p.analytic_ptr(api.ptr(x), out, batch), 2, real),
             l2_call("envelope", hilbert_truth.envelope(xh), rdt(real), lambda p, out: p.envelope_ptr(api.ptr(x), out, batch), 2, real)]
    compare(api, real, "hilbert", f"n={n}", make, "hilbert one-launch: ", [(xh, x)], calls, one_launch_bounds(batch))


CZT_BASE = {"f32": 4e-6, "f64": 1e-11}  # tests/czt_cases.py's BASE


def czt_calls(api, real, n, m, real_input, batch, x, xh, pars):
    want = czt_truth.czt(xh, m, *pars)
    bound = CZT_BASE[real] * czt_truth.chirp_ratio(n, m, pars[0], pars[2])
    return [Call("czt", (batch, m), cdt(real), lambda p, out: p.transform_ptr(api.ptr(x), out, batch), lambda got: rel_l2(got, want),
                 lambda d: bound)]


def czt_sweep(api, real, n, m, real_input):
    """CztPlan::sweep (czt_in: user rows of n -> work rows of L; czt_out: work rows of L -> user rows of m) and ::multiply (where the
    composed route convolves by forward, product, inverse) on "fusion" = 0.  row = L complex values, L = next_pow2(n + m - 1); scratch
    per row L complex values, three times that where the convolution runs as fused passes (read off the describe string).  The zoom
    arc of tests/czt_cases.py; bound: its BASE x chirp_ratio."""
    rng = np.random.default_rng(15 + n + m)
    pars = (1.0, -0.1 / m, 1.0, 0.2)
    xh = czt_truth.rows(rng, BATCH, n, rdt(real) if real_input else cdt(real))
    x = api.put(xh)
    L = 1 << (n + m - 2).bit_length()

    def make(fa):
        p = fa.Czt(n, m, *pars, real, real_input)
        p.set_option("fusion", 0)
        return p
    d = api.create(make).describe()
    per = (3 if "conv fused passes" in d else 1) * L * elem(real)
    compare(api, real, "czt", f"n={n} m={m} {'real' if real_input else 'complex'}", make, "czt composed: ", [(xh, x)],
            czt_calls(api, real, n, m, real_input, BATCH, x, xh, pars), byte_bounds(L * elem(real), per, "FOURIER_CZT_SCRATCH_BYTES"))
    return d


def czt_one_launch(api, real):
    """CztPlan::transform on the one-launch route (n = m = 1000, L = 2048, the default there): launches of FOURIER_LAUNCH_ITEMS rows"""
    n = m = 1000
    batch = 5
    rng = np.random.default_rng(16)
    pars = (1.0, -0.1 / m, 1.0, 0.2)
    xh = czt_truth.rows(rng, batch, n, cdt(real))
    x = api.put(xh)
    compare(api, real, "czt", f"n={n} m={m}", lambda fa: fa.Czt(n, m, *pars, real, False), "czt one-launch: ", [(xh, x)],
            czt_calls(api, real, n, m, False, batch, x, xh, pars), one_launch_bounds(batch))


def resample_sweep(api, real, n, m, complex_rows, fusion):
    """ResamplePlan::sweep: the remap of complex rows (rows of n -> rows of m, written into the CALLER's output), its half-spectrum
    form on the composed real route (rows of n / 2 + 1 -> m / 2 + 1) and the fused untangle (rows of n / 2 -> m / 2; n and m even).
    row = the larger side; scratch per row n complex values, real rows n / 2 + 1 + m / 2 + 1.  With a window.  tol():
    test_gpu_resample.py's, twice the base."""
    rng = np.random.default_rng(17 + 1000 * n + m)
    xh = resample_truth.rows(rng, BATCH, n, rdt(real), complex_rows)
    wh = resample_truth.window(rng, n, rdt(real))
    x, w = api.put(xh), api.put(wh)
    if complex_rows:
        route, ivals, ovals, per = "complex", n, m, n * elem(real)
    else:
        route = "real fused untangle" if fusion else "real composed"
        ivals, ovals = (n // 2, m // 2) if fusion else (n // 2 + 1, m // 2 + 1)
        per = (n // 2 + 1 + m // 2 + 1) * elem(real)

    def make(fa):
        p = fa.Resample(n, m, real, real_input=not complex_rows)
        p.set_option("fusion", fusion)
        p.set_window_ptr(api.ptr(w))
        return p
    calls = [l2_call("resample", resample_truth.resample(xh, m, wh), xh.dtype, lambda p, out: p.forward_ptr(api.ptr(x), out, BATCH), 2, real)]
    compare(api, real, "resample", f"{n}->{m} {route}", make, f"resample {route}: ", [(xh, x), (wh, w)], calls,
            byte_bounds(max(ivals, ovals) * elem(real), per, "FOURIER_RESAMPLE_SCRATCH_BYTES"))


def conv_want(x, h):
    """numpy in f64; row b with filter b mod F (tests/test_gpu_conv.py's want)"""
    n = x.shape[-1]
    hb = h[np.arange(x.shape[0]) % h.shape[0]]
    if np.iscomplexobj(x):
        return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * np.fft.fft(hb.astype(np.complex128), n, axis=-1), axis=-1)
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * np.fft.rfft(hb.astype(np.float64), n, axis=-1), n=n, axis=-1)


def conv_sweep(api, real, n, real_data, fusion):
    """ConvPlan::sweep with three filters and 7 rows: the filter a launch starts on is a.first = (b0 + r0) % 3, non-zero on later
    launches wherever rows_per is no multiple of 3 (one, two and -- "ragged" -- three rows a launch: firsts 0 1 2 0 1 2 0, 0 2 1 0 under
    the scratch bound, 0 0 0).  Complex rows on the composed route (len = n), real rows on the fused untangle route (len = n / 2, even
    n) and on the composed one (len = n / 2 + 1).  Scratch per row: n complex values, real rows n / 2 + 1.  tol(): test_gpu_conv.py's,
    three times the base."""
    rng = np.random.default_rng(18 + n + 2 * real_data + fusion)
    F, taps = 3, 9
    dt = rdt(real) if real_data else cdt(real)
    xh, hh = randn(rng, (BATCH, n), dt), randn(rng, (F, taps), dt)
    x, h = api.put(xh), api.put(hh)
    if real_data:
        route, length = ("conv real fused untangle: ", n // 2) if fusion else ("conv real composed: ", n // 2 + 1)
        per = (n // 2 + 1) * elem(real)
    else:
        route, length, per = "conv composed: ", n, n * elem(real)
    # the filters the launches of the second-chunk case start on: chunks of 4 and 3 rows, launches of 2
    firsts = [(c0 + r0) % F for c0, nb in chunks_of(BATCH, 4) for r0, _ in chunks_of(nb, 2)]
    assert firsts == [0, 2, 1, 0] and [r0 % F for r0, _ in chunks_of(BATCH, 1)] == [0, 1, 2, 0, 1, 2, 0]

    def make(fa):
        p = fa.FftConv(n, real, real_data)
        p.set_option("fusion", fusion)
        p.set_filters_ptr(api.ptr(h), taps, F)
        return p
    calls = [l2_call("apply", conv_want(xh, hh), dt, lambda p, out: p.apply_ptr(api.ptr(x), out, BATCH), 3, real)]
    compare(api, real, "conv", f"n={n} {route}", make, route, [(xh, x), (hh, h)], calls, byte_bounds(length * elem(real), per, CONV))


def xcorr_sweep(api, real, n, L, real_data):
    """XcorrPlan::sweep on the composed route: pad (rows of n -> rows of L), the product of the spectra (rows of L / 2 + 1, complex rows
    L) and the lag window (rows of L -> rows of `lags`), each with its own rows_per = bound // max(input row, output row).  The bounds are
    in units of the largest row of the three, L values of the handle's kind or the spectrum row; scratch per row pair as row_bytes()
    states it.  Window (-5, 21): all three sweeps run.  Bound: test_gpu_xcorr.py's, 4 x base on the window error."""
    rng = np.random.default_rng(19 + n + L)
    first, lags = -5, 21
    dt = rdt(real) if real_data else cdt(real)
    xh, yh = xcorr_truth.rows(rng, BATCH, n, dt), xcorr_truth.rows(rng, BATCH, n, dt)
    x, y = api.put(xh), api.put(yh)
    vs = elem(real) // 2 if real_data else elem(real)
    spec = (L // 2 + 1) * elem(real) if real_data else L * elem(real)
    per = 2 * (L // 2 + 1) * elem(real) + 3 * L * vs if real_data else 2 * L * elem(real)
    row = max(spec, L * vs)
    want = xcorr_truth.full(xh, yh, L)

    def make(fa):
        p = fa.CrossCorrelation(n, L, first, lags, real, real_data)
        p.set_option("fusion", 0)
        return p
    bounds = byte_bounds(row, per, "FOURIER_XCORR_SCRATCH_BYTES")
    for _, env in bounds:  # the three sweeps under every bound: each takes more than one launch
        for irow, orow in ((n * vs, L * vs), (spec, spec), (L * vs, lags * vs)):
            assert len(sizes(BATCH, max(1, env[BYTES] // max(irow, orow)))) > 1
    calls = [Call("correlate", (BATCH, lags), dt, lambda p, out: p.correlate_ptr(api.ptr(x), api.ptr(y), out, BATCH),
                  lambda got: xcorr_truth.window_err(got, want, first, lags), lambda d: 4 * base(d, real))]
    compare(api, real, "xcorr", f"n={n} L={L} {'real' if real_data else 'complex'}", make, "xcorr composed: ", [(xh, x), (yh, y)], calls, bounds)


def xcorr_one_launch(api, real, switches):
    """XcorrPlan::correlate on the one-launch route (real rows, L = 2048, n = 1024, the full lag window): launches of
    FOURIER_LAUNCH_ITEMS row pairs, the pointer steps of x, y and the output.  `switches`: what selects a kernel for this precision
    in the caller's library (tests/test_gpu_xcorr.py's make())."""
    n, L, batch = 1024, 2048, 5
    rng = np.random.default_rng(20)
    xh, yh = xcorr_truth.rows(rng, batch, n, rdt(real)), xcorr_truth.rows(rng, batch, n, rdt(real))
    x, y = api.put(xh), api.put(yh)
    want = xcorr_truth.full(xh, yh, L)
    calls = [Call("correlate", (batch, L), rdt(real), lambda p, out: p.correlate_ptr(api.ptr(x), api.ptr(y), out, batch),
                  lambda got: xcorr_truth.window_err(got, want, 0, L), lambda d: 4 * base(d, real))]
    compare(api, real, "xcorr", f"n={n} L={L}", lambda fa: fa.CrossCorrelation(n, L, 0, L, real, True), "xcorr one-launch: ",
            [(xh, x), (yh, y)], calls, one_launch_bounds(batch), always=switches)


# ---- linear convolution: LAUNCH_WORKGROUPS
def lconv_want(x, h, mode):
    """numpy.convolve in f64, row b with filter b mod F, sliced as include/fourier.h says (tests/test_gpu_lconv.py's want)"""
    lx, k = x.shape[-1], h.shape[-1]
    wide = np.complex128 if np.iscomplexobj(x) else np.float64
    off, lout = {"full": (0, lx + k - 1), "valid": (k - 1, lx - k + 1)}[mode]
    return np.array([np.convolve(x[b].astype(wide), h[b % h.shape[0]].astype(wide))[off:off + lout] for b in range(x.shape[0])])


def lconv_split(api, real, real_data, overlap_save):
    """LinearConvPlan::apply on the overlap-save route (blocks of 2048: wpr workgroups a row, one per block, real rows one per pair of
    blocks; launches of max(1, items // wpr) rows, the filter of a row counted from b0) and ::copy_rows on the padded route
    ("overlap_save" = 0, M = 8192: segs = ceil(row words / 2048) workgroups a row, for the copy in and the copy out).  Lx = 5000, K = 129,
    two filters, five rows: one row per launch, two (ragged), and a bound of one workgroup (below a row).  Under a scratch of two rows
    the padded route splits inside three chunks.  tol(): test_gpu_lconv.py's, three times the base."""
    lx, k, batch, F, mode = 5000, 129, 5, 2, "full"
    rng = np.random.default_rng(21 + real_data)
    dt = rdt(real) if real_data else cdt(real)
    xh, hh = randn(rng, (batch, lx), dt), randn(rng, (F, k), dt)
    x, h = api.put(xh), api.put(hh)
    lout = lx + k - 1
    words = 1 if real_data else 2
    if overlap_save:
        step = (2048 - (k - 1)) // 64 * 64  # LINE = 64 values: the blocks advance by whole lines
        blocks = -(-lout // step)
        per_row = (blocks + 1) // 2 if real_data else blocks
        prefix = f"lconv overlap-save: block 2048 step {step} blocks {blocks}"
    else:
        per_row = -(-8192 * words // LCONV_SEG)  # the copy in writes rows of M words; the copy out (rows of lout words) takes fewer
        prefix = "lconv padded: M=8192, "
    bounds = [("one row", {ITEMS: per_row}), ("ragged", {ITEMS: 2 * per_row + 1}), ("below a row", {ITEMS: 1})]
    assert [sizes(batch, max(1, env[ITEMS] // per_row)) for _, env in bounds] == [[1] * 5, [2, 2, 1], [1] * 5]
    if not overlap_save:
        row = 8192 * (elem(real) // 2 if real_data else elem(real))
        bounds.append(("inside every chunk", {ITEMS: per_row, CONV: 2 * row}))
        assert [sizes(nb, 1) for nb in sizes(batch, chunk_rows(batch, 2 * row, row))] == [[1, 1], [1, 1], [1]]

    def make(fa):
        p = fa.LinearConv(lx, k, real, mode, real_data)
        p.set_option("overlap_save", overlap_save)
        p.set_filters_ptr(api.ptr(h), F)
        return p
    calls = [l2_call("apply", lconv_want(xh, hh, mode), dt, lambda p, out: p.apply_ptr(api.ptr(x), out, batch), 3, real)]
    compare(api, real, "lconv", f"{'real' if real_data else 'complex'} {'overlap-save' if overlap_save else 'padded'}", make, prefix,
            [(xh, x), (hh, h)], calls, bounds)


# ---- the fused frame routes: LAUNCH_ITEMS frames of the flat frame index
def frame_bounds(total, tile):
    """launches of one frame (a short call), and of tile + 5 frames: no multiple of the kernel's frames per workgroup, so every later
    launch begins inside what would have been a tile, and the last one is ragged"""
    k = tile + 5
    walk = chunks_of(total, k)
    assert len(walk) > 1 and walk[1][0] % tile != 0 and walk[-1][1] != k, walk
    return [("ragged, inside a tile", {ITEMS: k})]


def one_frame_bounds(total):
    assert len(chunks_of(total, 1)) == total > 1
    return [("one frame", {ITEMS: 1})]


def frame_shape(real, hop, frames=None):
    """rows of tile + 3 frames at n_fft = 256 under reflect padding, an odd row length"""
    fr = FUSED_TILE[real] + 3 if frames is None else frames
    return fr, (fr - 1) * hop + 3


def stft_frames(api, real, frames=None):
    """StftPlan::forward on the fused route (n_fft 256, hop 64, reflect): 3 rows of tile + 3 frames in launches of tile + 5 frames, and
    3 rows of 5 frames one frame a launch.  tol(): test_gpu_stft.py's, twice the base."""
    n, hop, batch = 256, 64, 3
    fr, length = frame_shape(real, hop, frames)
    rng = np.random.default_rng(31 + fr)
    xh, wh = randn(rng, (batch, length), rdt(real)), uniform(rng, real, n)
    x, w = api.put(xh), api.put(wh)
    assert stft_truth.frames(length, n, hop, "reflect") == fr

    def make(fa):
        p = fa.Stft(n, real, hop, None, True, "reflect")
        p.set_window_ptr(api.ptr(w))
        return p
    calls = [l2_call("forward", stft_truth.stft(xh, n, hop, n, wh, "reflect"), cdt(real),
                     lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch), 2, real)]
    bounds = frame_bounds(batch * fr, FUSED_TILE[real]) if frames is None else one_frame_bounds(batch * fr)
    compare(api, real, "stft", f"frames={fr}", make, "stft fused rows, istft composed: ", [(xh, x), (wh, w)], calls, bounds)


def spectrogram_frames(api, real, frames=None):
    """SpectrogramPlan::forward on the fused route ("fusion" = 1), the shapes of stft_frames; power and magnitude.  tol():
    test_gpu_spectrogram.py's, four times the base."""
    n, hop, batch = 256, 64, 3
    fr, length = frame_shape(real, hop, frames)
    rng = np.random.default_rng(32 + fr)
    xh, wh = randn(rng, (batch, length), rdt(real)), uniform(rng, real, n)
    x, w = api.put(xh), api.put(wh)

    def make(fa):
        p = fa.Spectrogram(n, real, hop, None, True, "reflect")
        p.set_option("fusion", 1)
        p.set_window_ptr(api.ptr(w))
        return p
    calls = [l2_call(f"power={power}", spectrogram_truth.spectrogram(xh, n, hop, n, wh, "reflect", power, power == 1), rdt(real),
                     lambda p, out, power=power: p.forward_ptr(api.ptr(x), out, length, batch, power, power == 1), 4, real)
             for power in (2, 1)]
    bounds = frame_bounds(batch * fr, FUSED_TILE[real]) if frames is None else one_frame_bounds(batch * fr)
    compare(api, real, "spectrogram", f"frames={fr}", make, "spectrogram fused rows, welch fused rows: ", [(xh, x), (wh, w)], calls, bounds)


def bandspec_frames(api, real, frames=None):
    """BandSpecPlan::forward on the fused route, the shapes of stft_frames, a random dense band matrix of 24 bands with negative
    entries.  Figure and bound: tests/bandspec_cases.py's -- the error over the norm of the |W| |X|^p sums, four times the base."""
    n, hop, batch, bands = 256, 64, 3, 24
    fr, length = frame_shape(real, hop, frames)
    rng = np.random.default_rng(33 + fr)
    xh, wh = randn(rng, (batch, length), rdt(real)), uniform(rng, real, n)
    W = np.ascontiguousarray(rng.standard_normal((bands, n // 2 + 1)).astype(rdt(real)))
    x, w = api.put(xh), api.put(wh)
    want = bandspec_truth.band_spectrogram(xh, W.astype(np.float64), n, hop, n, wh, "reflect", 2, False)
    scale = float(np.linalg.norm(bandspec_truth.abs_band_spectrogram(xh, W.astype(np.float64), n, hop, n, wh, "reflect", 2, False)))

    def make(fa):
        p = fa.BandSpectrogram(n, bands, real, hop, None, True, "reflect")
        p.set_option("fusion", 1)
        p.set_window_ptr(api.ptr(w))
        p.set_bands_ptr(W.ctypes.data)  # a host address on either side
        return p
    calls = [Call("forward", want.shape, rdt(real), lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch, 2, False),
                  lambda got: float(np.linalg.norm(got - want)) / scale, lambda d: 4 * base(d, real))]
    bounds = frame_bounds(batch * fr, FUSED_TILE[real]) if frames is None else one_frame_bounds(batch * fr)
    compare(api, real, "bandspec", f"frames={fr}", make, "bandspec fused rows: ", [(xh, x), (wh, w)], calls, bounds)


def mdct_frames(api, real, frames=None):
    """MdctPlan::forward on the fused route ("fusion" = 1; n = 256 coefficients a frame, centred, the sine window): rows of tile + 3
    frames in launches of tile + 5 (odd: no multiple of any power-of-two frames per workgroup), and rows of 5 frames one frame a launch.  tol(): test_gpu_mdct.py's, twice the base."""
    n, batch = 256, 3
    fr = FUSED_TILE[real] + 3 if frames is None else frames
    length = mdct_truth.default_length(fr, n, True) - 3
    assert mdct_truth.frames(length, n, True) == fr
    rng = np.random.default_rng(34 + fr)
    xh = randn(rng, (batch, length), rdt(real))
    x = api.put(xh)
    calls = [l2_call("forward", mdct_truth.mdct(xh, n, None, True), rdt(real), lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch),
                     2, real)]
    bounds = frame_bounds(batch * fr, FUSED_TILE[real]) if frames is None else one_frame_bounds(batch * fr)

    def make(fa):
        p = fa.Mdct(n, real, True)
        p.set_option("fusion", 1)
        return p
    compare(api, real, "mdct", f"frames={fr}", make, "mdct fused rows, imdct composed: ", [(xh, x)], calls, bounds)


def pfb_frames(api, real, real_input, frames=None):
    """PfbPlan::forward on the fused route (256 channels, 4 taps, hop 192), real and complex rows.  tol(): test_gpu_pfb.py's, twice the
    base."""
    P, T, D, batch = 256, 4, 192, 3
    fr = FUSED_TILE[real] + 3 if frames is None else frames
    length = (fr - 1) * D + P * T + 5
    assert pfb_truth.frames(length, P, T, D) == fr
    rng = np.random.default_rng(35 + fr + real_input)
    dt = rdt(real) if real_input else cdt(real)
    xh, hh = randn(rng, (batch, length), dt), uniform(rng, real, P * T)
    x, h = api.put(xh), api.put(hh)

    def make(fa):
        p = fa.Pfb(P, T, real, D, real_input)
        p.set_filter_ptr(api.ptr(h))
        return p
    calls = [l2_call("forward", pfb_truth.pfb(xh, hh, P, T, D, real_input), cdt(real),
                     lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch), 2, real)]
    # the kernel's frames per workgroup depend on the input kind; tile + 5 is odd at either precision, so no power of two divides it
    total, k = batch * fr, FUSED_TILE[real] + 5
    walk = chunks_of(total, k if frames is None else 1)
    assert len(walk) > 1 and (frames is not None or (k % 2 == 1 and walk[-1][1] != k))
    compare(api, real, "pfb", f"{'real' if real_input else 'complex'} frames={fr}", make, "pfb fused rows: ", [(xh, x), (hh, h)], calls,
            [("ragged, inside a tile", {ITEMS: k})] if frames is None else [("one frame", {ITEMS: 1})])


def composed_frames(api, real):
    """The composed frame routes cap a chunk of the scratch at the same bound (min(chunk_rows(...), items) in StftPlan::prepare_forward,
    MdctPlan::prepare_forward and ::inverse_chunks, PfbPlan::prepare): "fusion" = 0, n = 64, 3 rows of 10 or 11 frames under a bound of 7
    frames -- chunks that end inside rows, the last one ragged -- and the MDCT's inverse, whose ranges then hold 7 frames of the
    scratch.  Tolerances: the forward and inverse ones of test_gpu_stft.py, test_gpu_mdct.py and test_gpu_pfb.py."""
    n, batch, items = 64, 3, 7
    rng = np.random.default_rng(39)
    length = 9 * n + 5
    xh, wh, w2h = randn(rng, (batch, length), rdt(real)), uniform(rng, real, n), uniform(rng, real, 2 * n)
    x, w, w2 = api.put(xh), api.put(wh), api.put(w2h)
    bounds = [("chunks of 7 frames", {ITEMS: items})]

    def stft(fa):
        p = fa.Stft(n, real, n // 4, None, True, "reflect")
        p.set_option("fusion", 0)
        p.set_window_ptr(api.ptr(w))
        return p
    fr = stft_truth.frames(length, n, n // 4, "reflect")
    assert len(chunks_of(batch * fr, items)) > 1 and fr % items != 0
    compare(api, real, "stft", "composed", stft, "stft composed, istft composed: ", [(xh, x), (wh, w)],
            [l2_call("forward", stft_truth.stft(xh, n, n // 4, n, wh, "reflect"), cdt(real),
                     lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch), 2, real)], bounds)

    def mdct(fa):
        p = fa.Mdct(n, real, True)
        p.set_option("fusion", 0)
        p.set_window_ptr(api.ptr(w2))
        return p
    fr = mdct_truth.frames(length, n, True)
    back = min(length, mdct_truth.default_length(fr, n, True)) - 5
    Xh = mdct_truth.mdct(xh, n, w2h, True).astype(rdt(real))
    X = api.put(np.ascontiguousarray(Xh))
    assert len(chunks_of(batch * fr, items)) > 1 and fr > items
    compare(api, real, "mdct", "composed", mdct, "mdct composed, imdct composed: ", [(xh, x), (w2h, w2), (Xh, X)],
            [l2_call("forward", mdct_truth.mdct(xh, n, w2h, True), rdt(real), lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch), 2, real),
             l2_call("inverse", mdct_truth.imdct(Xh, n, back, w2h, True), rdt(real),
                     lambda p, out: p.inverse_ptr(api.ptr(X), out, fr, back, batch), 4, real)], bounds)
    P, T, D = 64, 4, 40
    hh = uniform(rng, real, P * T)
    h = api.put(hh)

    def pfb(fa):
        p = fa.Pfb(P, T, real, D, True)
        p.set_option("fusion", 0)
        p.set_filter_ptr(api.ptr(h))
        return p
    fr = pfb_truth.frames(length, P, T, D)
    assert len(chunks_of(batch * fr, items)) > 1 and fr % items != 0
    compare(api, real, "pfb", "composed", pfb, "pfb composed: ", [(xh, x), (hh, h)],
            [l2_call("forward", pfb_truth.pfb(xh, hh, P, T, D, True), cdt(real), lambda p, out: p.forward_ptr(api.ptr(x), out, length, batch),
                     2, real)], bounds)


# ---- Welch and cross-spectrum row groups: min(..., LAUNCH_ITEMS / max(frames, tiles x 32))
def group_case(real, fused, pair):
    """frames a row, slots of partials a row, and the bound that gives groups of two rows of a batch of five"""
    if fused:
        tile = FUSED_TILE[real] // (2 if pair else 1)
        fr = tile + 3
    else:
        tile, fr = WELCH_TILE, 2 * WELCH_TILE  # every row, and with it every launch of the composed walk, ends on a slot
    tiles = -(-fr // tile)
    items = 2 * max(fr, tiles * WELCH_TILE)
    assert sizes(5, max(1, items // max(fr, tiles * WELCH_TILE))) == [2, 2, 1]
    return fr, tiles, items


def welch_groups(api, real, fused):
    """SpectrogramPlan::prepare_partials: five rows in groups of 2, 2 and 1 through one partials buffer, on the fused route (n_fft 256,
    tile + 3 frames a row) and on the composed one (n_fft 64, 64 frames a row: the frame chunks, which the same bound caps at 128
    frames, end on row ends, so no slot of partials is split and the sum keeps its order).  A second bound adds a scratch bound of
    three rows of partials: the launch term is the smaller one.  tol(): test_gpu_spectrogram.py's."""
    n = 256 if fused else 64
    hop, batch = n // 4, 5
    fr, tiles, items = group_case(real, fused, False)
    length = (fr - 1) * hop + 3
    rng = np.random.default_rng(36 + fused)
    xh, wh = randn(rng, (batch, length), rdt(real)), uniform(rng, real, n)
    x, w = api.put(xh), api.put(wh)
    assert stft_truth.frames(length, n, hop, "reflect") == fr
    part_row = tiles * (n // 2 + 1) * (elem(real) // 2)
    frame = (n // 2 + 1) * elem(real) + n * (elem(real) // 2)
    scratch = max(3 * part_row, 2 * fr * frame)  # three rows of partials, and (composed) the two rows of frames of a group
    assert chunk_rows(batch, scratch, part_row) >= 3 and (fused or chunk_rows(2 * fr, scratch, frame) == 2 * fr)

    def make(fa):
        p = fa.Spectrogram(n, real, hop, None, True, "reflect")
        p.set_option("fusion", int(fused))
        p.set_window_ptr(api.ptr(w))
        return p
    route = "fused rows" if fused else "composed"
    calls = [l2_call("welch", spectrogram_truth.welch(xh, n, hop, n, wh, "reflect", True, 0.37), rdt(real),
                     lambda p, out: p.welch_ptr(api.ptr(x), out, length, batch, True, 0.37), 4, real)]
    compare(api, real, "welch", f"{route} frames={fr}", make, f"spectrogram {route}, welch {route}: ", [(xh, x), (wh, w)], calls,
            [("groups of two rows", {ITEMS: items}), ("groups of two rows, scratch of three", {ITEMS: items, REAL: scratch})])


def csd_groups(api, real, fused):
    """CsdPlan::prepare_partials and ::prepare_frames (frame pairs per chunk: min(..., LAUNCH_ITEMS / 2)), the cases of welch_groups:
    on the composed route the bound of 128 frames caps a chunk at 64 frame pairs, one row; the second bound adds a scratch bound of three
    rows of partials.  tol(): test_gpu_csd.py's, 4 x and 12 x its base()."""
    n = 256 if fused else 64
    hop, batch = n // 4, 5
    fr, tiles, items = group_case(real, fused, True)
    length = (fr - 1) * hop + 3
    rng = np.random.default_rng(37 + fused)
    xh, yh = csd_truth.pair(rng, batch, length, rdt(real))
    wh = uniform(rng, real, n)
    x, y, w = api.put(xh), api.put(yh), api.put(wh)
    assert fused or sizes(2 * fr, items // 2) == [fr, fr]
    part_row = tiles * CSD_PLANES * (n // 2 + 1) * (elem(real) // 2)
    pair = 2 * ((n // 2 + 1) * elem(real) + n * (elem(real) // 2))
    scratch = max(3 * part_row, 2 * fr * pair)  # three rows of partials, and (composed) the frame pairs of two rows
    assert chunk_rows(batch, scratch, part_row) >= 3 and (fused or chunk_rows(2 * fr, scratch, pair) >= fr)

    def make(fa):
        p = fa.CrossSpectrum(n, real, hop, None, True, "reflect")
        p.set_option("fusion", int(fused))
        p.set_window_ptr(api.ptr(w))
        return p

    def csd_base(d):
        blu = "bluestein" in d
        return (4e-6 if blu else 2e-6) if real == "f32" else (2e-13 if blu else 1e-13)
    route = "fused rows" if fused else "composed"
    want_p, want_c = csd_truth.csd(xh, yh, n, hop, n, wh, "reflect", True, 0.37), csd_truth.coherence(xh, yh, n, hop, n, wh, "reflect")
    calls = [Call("csd", want_p.shape, cdt(real), lambda p, out: p.csd_ptr(api.ptr(x), api.ptr(y), out, length, batch, True, 0.37),
                  lambda got: rel_l2(got, want_p), lambda d: 4 * csd_base(d)),
             Call("coherence", want_c.shape, rdt(real), lambda p, out: p.coherence_ptr(api.ptr(x), api.ptr(y), out, length, batch),
                  lambda got: rel_l2(got, want_c), lambda d: 12 * csd_base(d))]
    compare(api, real, "csd", f"{route} frames={fr}", make, f"csd {route}, coherence {route}: ", [(xh, x), (yh, y), (wh, w)], calls,
            [("groups of two rows", {ITEMS: items}), ("groups of two rows, scratch of three", {ITEMS: items, REAL: scratch})])


# ---- the synthesis bank's gather
def gather_pieces(walk, items):
    """the launches of IpfbPlan::gather over the chunks of a call (ipfb_truth.inverse_walk): (first row, rows, first sample, samples)"""
    return [(b0 + r0, nr, t0 + s0, ns) for b0, nb, t0, span, _, _ in walk for s0, ns in chunks_of(span, items)
            for r0, nr in chunks_of(nb, max(1, items // ns))]


def ipfb_gather(api, real, real_output, hop):
    """IpfbPlan::gather: 16 channels, 4 taps, hop 12 (< channels) and 20 (> channels), 9 frames, 3 rows of an odd length, real and
    complex output.  Bounds: 37 (pieces of 37 samples of a range, one row a launch: fb, e0, q0 and kcount recomputed per piece, and
    -- real rows of an odd length -- `pairs` changing from row to row); twice the length and three (the whole range, rows 2 + 1);
    one (a sample a launch); and 37 under a scratch of cover() + 1 frames (ranges inside every row, pieces inside every range).  tol():
    test_gpu_ipfb.py's, twice the base."""
    P, T, nf, batch = 16, 4, 9, 3
    length = ipfb_truth.full(nf, P, T, hop) - 5
    assert length % 2 == 1
    rng = np.random.default_rng(38 + hop + real_output)
    bins = P // 2 + 1 if real_output else P
    Yh, gh = randn(rng, (batch, nf, bins), cdt(real)), uniform(rng, real, P * T)
    Y, g = api.put(Yh), api.put(gh)
    vs = elem(real) // 2 if real_output else elem(real)
    fit = ipfb_truth.cover(P, T, hop) + 1
    whole = ipfb_truth.inverse_walk(P, T, hop, nf, batch, length, 1 << 40)
    ranges = ipfb_truth.inverse_walk(P, T, hop, nf, batch, length, fit)
    assert whole == [(0, batch, 0, length, 0, nf)] and len(ranges) > batch
    pieces = gather_pieces(whole, 37)
    assert pieces[:batch] == [(r, 1, 0, 37) for r in range(batch)] and pieces[-1][3] == length % 37 != 0
    assert [(p[0], p[1]) for p in gather_pieces(whole, 2 * length + 3)] == [(0, 2), (2, 1)]
    assert len(gather_pieces(whole, 1)) == batch * length and len(gather_pieces(ranges, 37)) > len(ranges)

    def make(fa):
        p = fa.Ipfb(P, T, real, hop, real_output)
        p.set_filter_ptr(api.ptr(g))
        return p
    calls = [l2_call("inverse", ipfb_truth.synth(Yh, gh, P, T, hop, real_output, length), rdt(real) if real_output else cdt(real),
                     lambda p, out: p.inverse_ptr(api.ptr(Y), out, nf, length, batch), 2, real)]
    compare(api, real, "ipfb", f"hop={hop} {'real' if real_output else 'complex'}", make, "ipfb composed: ", [(Yh, Y), (gh, g)], calls,
            [("pieces of 37 samples", {ITEMS: 37}), ("rows 2 + 1", {ITEMS: 2 * length + 3}), ("one sample", {ITEMS: 1}),
             ("pieces inside ranges", {ITEMS: 37, REAL: fit * P * vs})])
