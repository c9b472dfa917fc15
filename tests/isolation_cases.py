"""A non-finite value stays where the definition puts it: the table of tests/amplitude_cases.py once more, stated once and run twice --
on the CPU emulation (tests/test_isolation_emu.py) and on the MI355X (tests/test_gpu_isolation.py).  Every accuracy test feeds finite
noise and every guard band holds a finite sentinel, so a load from a neighbouring row, from beyond the input or from scratch an earlier
call left behind is invisible wherever the value is then multiplied by a zero window, a zero chirp or a zero pad: the result is right
to the last bit.  A NaN is not: 0 x NaN is NaN.

Nothing of a case is restated: CASES, and each case's make, routes, select, unit_inputs, rounded, run and truth, are amplitude_cases'.
What is here: how an output is cut into units, which units depend on a poisoned input, and the four checks.

Units.  A unit view (VIEWS) cuts an output, and its truth, into blocks of shape (units, elements); both have the same number of
units.  Rows by default; the two lag windows of a cross-correlation case, each with its rows; (call, row) where the leading axis of a
case is the call; the lines along the transformed axis of the strided-axis case; for check B (row, frame) of the forward frame handles
and the single output samples of the overlap-add inverses.  Every case is matched by exactly one rule, by the first word of its name
(view_of asserts it: a new family cannot fall into a default).

Dependence.  There is no map per family: the family's own f64 truth runs on the poisoned input, and a unit is DEPENDENT if any
element of it is non-finite there, CLEAN otherwise.  That gives filter b mod F, the delay-and-sum groups and the pairs of a
cross-correlation for free.

Checks, per case, route and precision, y0 the result of the same handle on the clean inputs (all of it finite).  Every comparison is
bit for bit (amplitude_cases.differing == 0 over the clean units); there is no tolerance in this file.
  A  a poisoned unit of any input: every input array of the case, every unit along its first axis in turn (the strided-axis case: one
     line, at every outer and the first, a middle and the last inner index), filled with NaN in both parts.  Every clean output unit
     equals y0; every dependent unit holds a non-finite value (STAYS_FINITE names the exceptions, with the reason).  Asserted before
     the handle runs: every poisoned run leaves a unit clean, and over the poisons of one input every output unit is clean once.
  B  one poisoned sample, the frame handles only: x[1, t] = +Inf, or for the inverses the whole input frame (1, f), at the first, a
     middle and the last position -- and, forward, at the first sample past the middle that lies directly behind some frame's span,
     where a gather one sample too long shows.  Clean units equal y0, dependent units are non-finite (of an inverse: every dependent
     sample).
     Asserted before the handle runs: the number of dependent units is the one the framing gives -- the frames whose padded support
     holds an image of t; the support of one frame clipped to the output -- so a truth that marked a whole row would fail here.
     MIDDLE states those counts at the middle position for the shapes of the table.  Welch, the cross spectrum and the coherence
     average over frames and the overlap-save blocks of LinearConv spread a NaN over a block np.convolve does not model: rows, check A.
  C  foreign memory: Banded places every input inside one allocation between two bands of NaN, each at least one unit and 64 elements
     long and a multiple of 256 bytes, so the data is aligned as in the plain placement.  The clean inputs placed so give y0.  On the
     device both bands are part of the same allocation as the data: a stray read is seen, not faulted on.
  D  no memory of the last call: after the last poisoned run of A, and of B, the clean inputs on the same handle give y0 -- a NaN left
     in plan-owned scratch or in a pad region a later call takes for zero.

A test prints one line -- the case, how many units were compared clean and how many were dependent per check, the routes -- and then
asserts everything."""
import collections

import numpy as np

import amplitude_cases as cases
import xcorr_truth

NAN, INF = float("nan"), float("inf")
BAND_ELEMENTS, BAND_BYTES = 64, 256


# ---- unit views: an array -> blocks of shape (units, elements)
def rows(ctx, a):
    return [a.reshape(a.shape[0], -1)]


def two_axes(ctx, a):
    """(call, row) of a case whose leading axis is the call; (row, frame) of a frame-major output"""
    return [a.reshape(a.shape[0] * a.shape[1], -1)]


def samples(ctx, a):
    return [a.reshape(-1, 1)]


def lines(ctx, a):
    """(outer, n, inner) -> the outer x inner lines along the transformed axis"""
    return [np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, a.shape[1])]


def lag_windows(ctx, a):
    """the output of a cross-correlation case: its lag windows one after the other, each ctx.batch rows"""
    blocks, at = [], 0
    for p in ctx.plan.plans:
        blocks.append(a[at:at + ctx.batch * p.lags()].reshape(ctx.batch, p.lags()))
        at += ctx.batch * p.lags()
    assert at == a.size
    return blocks


def windowed_lags(ctx, r):
    """the truth of a cross-correlation case, all L lags: the same windows of it"""
    return [xcorr_truth.window(r, first, lags) for first, lags in cases.xcorr_windows(r.shape[-1])]


def filled(a, value):
    return complex(value, value) if a.dtype.kind == "c" else value


def poison_rows(a):
    """check A's poisons of one input: every unit along the first axis in turn"""
    for b in range(a.shape[0]):
        p = a.copy()
        p[b] = filled(a, NAN)
        yield f"unit {b}", p


def poison_lines(a):
    """... of the strided-axis case: one line along the transformed axis, at every outer index and the first, a middle and the last
    inner one (the column-tile and lane kernels carry many inner lines in one tile)"""
    outer, _, inner = a.shape
    for o in range(outer):
        for i in sorted({0, inner // 2, inner - 1}):
            p = a.copy()
            p[o, :, i] = filled(a, NAN)
            yield f"line ({o}, {i})", p


# out, truth: the views of checks A, C and D; poisons: check A's poisons of one input; fine, forward, count: check B's view, whether
# the poison is a sample of a forward handle (else a frame of an inverse) and the count the framing gives (None: no check B)
View = collections.namedtuple("View", "families out truth poisons fine forward count", defaults=(poison_rows, None, None, None))


def poison_at(a, at):
    """check B: x[1, t] = +Inf of a forward frame handle, the whole input frame (1, f) = +Inf of an inverse"""
    p = a.copy()
    p[1, at] = filled(a, INF)
    return p


def framing(ctx, family):
    """(the samples a frame spans, the hop, the padding in front, whether the padding reflects), from the handle's own getters"""
    p = ctx.plan
    if family in ("stft", "istft", "spectrogram", "bandspec"):
        return p.n_fft(), p.hop(), p.n_fft() // 2, True
    if family in ("mdct", "imdct"):
        return 2 * p.size(), p.size(), p.size(), False  # centred: one hop of zeros in front
    return p.channels() * p.taps(), p.hop(), 0, False   # pfb, ipfb


def frames_holding(ctx, family, t, length, frames):
    """the frames f < frames whose span [f hop, f hop + span) of the padded row holds sample t or one of its mirror images (numpy's
    "reflect": x[pad - j] at j < pad in front, x[length - 2 - i] at the i-th position behind)"""
    span, hop, pad, reflect = framing(ctx, family)
    at = {pad + t}
    if reflect and 1 <= t <= pad:
        at.add(pad - t)
    if reflect and 0 <= length - 2 - t < pad:
        at.add(pad + length + (length - 2 - t))
    return sum(1 for f in range(frames) if any(f * hop <= j < f * hop + span for j in at))


def behind_a_frame(ctx, family, length):
    """the first sample past the middle that lies directly behind the span of some frame: a gather one sample too long reaches it"""
    span, hop, pad, _ = framing(ctx, family)
    return next(t for t in range(length // 2 + 1, length) if (t + pad - span) % hop == 0)


def samples_of_frame(ctx, family, f, length, frames):
    """the output samples t < length that frame f reaches: [f hop - pad, f hop - pad + span), clipped"""
    span, hop, pad, _ = framing(ctx, family)
    return max(0, min(length, f * hop - pad + span) - max(0, f * hop - pad))


VIEWS = (
    View(("fft", "rfft", "irfft", "rfftn", "irfftn", "fftconv", "lconv", "resample", "czt", "hilbert", "welch", "csd", "coherence", "delay",
          "cepstrum"), rows, rows),
    View(("r2r",), rows, rows),  # the truth covers pick(ctx, out), every row of it: the unit is still the row
    View(("xcorr", "gcc-phat"), lag_windows, windowed_lags),
    View(("convnd", "nufft"), two_axes, two_axes),
    View(("axis",), lines, lines, poison_lines),
    View(("stft", "spectrogram", "bandspec", "mdct", "pfb"), rows, rows, poison_rows, two_axes, True, frames_holding),
    View(("istft", "imdct", "ipfb"), rows, rows, poison_rows, samples, False, samples_of_frame),
)

# Dependent units that may stay finite, by case name, with the reason.  Only the second half of A and B is waived: the clean units of
# these cases are compared like everyone's.
STAYS_FINITE = {
    # kernels_bandspec.h finishes a band as log_mult ln(y > log_floor ? y : log_floor): the comparison is false for a NaN, so a
    # poisoned frame comes out as log_mult ln(log_floor), on the emulation as on the device.  The linear cases of the same kernels
    # are not exempt, and they share every load.
    "bandspec 256 20 bands power 1 log": "the floor's comparison is false for a NaN: the frame reads log_mult ln(log_floor)",
    "bandspec 256 20 bands power 2 log": "the floor's comparison is false for a NaN: the frame reads log_mult ln(log_floor)",
}
assert set(STAYS_FINITE) <= set(cases.NAMES)

# Check B's counts at the middle position for the shapes of the table, as the definitions give them: n_fft / hop frames, the two frames
# of an MDCT sample, ceil or floor of P T / D; one whole frame of an inverse.  frames_holding and samples_of_frame must give these.
MIDDLE = {"stft 256 hop 64": 4, "mdct 256": 2, "pfb P=256 T=4 D=192 real": 6, "pfb P=256 T=4 D=192 complex": 6,
          "istft 256 hop 64": 256, "imdct 256": 512, "ipfb P=256 T=4 D=192 real": 1024, "ipfb P=256 T=4 D=192 complex": 1024}
assert set(MIDDLE) <= set(cases.NAMES)


def family(case):
    return case.name.split()[0]


def view_of(case):
    found = [v for v in VIEWS if family(case) in v.families]
    assert len(found) == 1, (case.name, "is matched by", len(found), "unit-view rules")
    return found[0]


# ---- check C's placement
class Banded:
    """the adapter with every input between two bands of NaN inside ONE allocation of the adapter's side; the slice that comes back
    is the data, and api.ptr of it the data's address"""

    def __init__(self, api):
        self.api, self.fa, self.device, self.ptr, self.run = api, api.fa, api.device, api.ptr, api.run

    @staticmethod
    def band(a):
        """elements of one band: at least a unit of the first axis and BAND_ELEMENTS, rounded up to a multiple of BAND_BYTES"""
        per = BAND_BYTES // np.gcd(BAND_BYTES, a.itemsize)
        need = max(a[0].size if a.ndim > 1 else 1, BAND_ELEMENTS)
        return -(-need // per) * per

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.dtype.kind in "fc", a.dtype
        band = self.band(a)
        assert band >= BAND_ELEMENTS and band * a.itemsize % BAND_BYTES == 0
        whole = np.full(a.size + 2 * band, filled(a, NAN), a.dtype)
        whole[band:band + a.size] = a.ravel()
        return self.api.put(whole)[band:band + a.size]


# ---- comparing
def unit_count(blocks):
    return sum(b.shape[0] for b in blocks)


def dependent(blocks):
    """per unit: does it hold a non-finite value"""
    return np.concatenate([~np.isfinite(b).all(axis=1) for b in blocks])


class Report:
    """the figures of one test: ONE line, then everything is asserted"""

    def __init__(self, what):
        self.what, self.routes, self.failed = what, [], []
        self.counts = collections.OrderedDict()  # check -> [runs, clean units compared, dependent units]
        self.reals = 0                           # reals that differ from y0 in clean units

    def route(self, d):
        self.routes.append(d if not self.routes else d.split(":")[0].split(",")[0])

    def compare(self, check, where, view, ctx, y, y0, dep, must_be_non_finite):
        """the clean units of y against y0 bit for bit; the dependent ones hold a non-finite value"""
        got, want = view(ctx, y), view(ctx, y0)
        assert unit_count(got) == unit_count(want) == dep.size, (self.what, where, unit_count(got), dep.size)
        count = self.counts.setdefault(check, [0, 0, 0])
        count[0], count[1], count[2] = count[0] + 1, count[1] + int(np.count_nonzero(~dep)), count[2] + int(np.count_nonzero(dep))
        at = 0
        for g, w in zip(got, want):
            d = dep[at:at + g.shape[0]]
            at += g.shape[0]
            bad = cases.differing(g[~d], w[~d])
            self.reals += bad
            if bad:
                units = np.flatnonzero([cases.differing(g[u], w[u]) for u in np.flatnonzero(~d)])
                self.failed.append((check, where, f"{bad} reals of {units.size} clean units differ from the clean run, the first at clean unit {units[0]}"))
            finite = np.isfinite(g[d]).all(axis=1)
            if must_be_non_finite and finite.any():
                self.failed.append((check, where, f"{int(finite.sum())} of {int(d.sum())} dependent units are finite"))

    def print(self):
        parts = [f"{c}: {runs} runs, {clean} clean units compared, {dep} dependent" for c, (runs, clean, dep) in self.counts.items()]
        print(f"isolation {self.what}: " + "; ".join(parts) + f"; {self.reals} reals differ in clean units  [{' | '.join(self.routes)}]")

    def check(self):
        assert not self.failed, (self.what, self.failed)


def check_isolation(api, case, real):
    view = view_of(case)
    fam = family(case)
    ctx = case.make(api, real)
    ins = cases.rounded(case.unit_inputs(ctx), real)
    case.conditions(ctx, ins)
    case.hold(ctx, ins)
    strict = case.name not in STAYS_FINITE
    banded = Banded(api)
    rep = Report(f"{real} {case.name}")
    try:
        for options, prefix in case.routes(real):
            where = cases.opt(options)
            rep.route(case.select(ctx, real, options, prefix))
            y0 = case.run(api, ctx, ins)
            assert np.all(np.isfinite(y0)), (case.name, where, "the clean run is not finite")
            with np.errstate(all="ignore"):
                t0 = case.truth(ctx, ins)
            nobody = dependent(view.truth(ctx, t0))
            assert not nobody.any() and nobody.size == unit_count(view.out(ctx, y0)), (case.name, nobody.size)

            # C: the clean inputs between bands of NaN
            rep.compare("C", where, view.out, ctx, case.run(banded, ctx, ins), y0, nobody, False)

            # A: the poisons and what depends on each, by the truth; the conditions; then the handle
            runs = []
            for i, a in enumerate(ins):
                clean_once = np.zeros(nobody.size, bool)
                for label, p in view.poisons(a):
                    poisoned = ins[:i] + [p] + ins[i + 1:]
                    with np.errstate(all="ignore"):
                        dep = dependent(view.truth(ctx, case.truth(ctx, poisoned)))
                    assert dep.any() and not dep.all(), (case.name, where, i, label, int(dep.sum()), "of", dep.size, "units depend")
                    clean_once |= ~dep
                    runs.append((f"{where}input {i} {label}", poisoned, dep))
                assert clean_once.all(), (case.name, where, i, "units never clean:", np.flatnonzero(~clean_once))
            for label, poisoned, dep in runs:
                rep.compare("A", label, view.out, ctx, case.run(api, ctx, poisoned), y0, dep, strict)
            # D: the same handle on the clean inputs again
            rep.compare("D", where + "after A", view.out, ctx, case.run(api, ctx, ins), y0, nobody, False)

            # B: one sample, or one frame of an inverse, at frame granularity
            if view.fine is None:
                continue
            length = ins[0].shape[-1] if view.forward else y0.shape[-1]
            frames = t0.shape[1] if view.forward else ins[0].shape[1]
            positions = (0, length // 2, behind_a_frame(ctx, fam, length), length - 1) if view.forward else (0, frames // 2, frames - 1)
            if case.name in MIDDLE:
                assert view.count(ctx, fam, positions[1], length, frames) == MIDDLE[case.name], (case.name, MIDDLE[case.name])
            runs = []
            for at in positions:
                poisoned = [poison_at(ins[0], at)] + ins[1:]
                with np.errstate(all="ignore"):
                    dep = dependent(view.fine(ctx, case.truth(ctx, poisoned)))
                want = view.count(ctx, fam, at, length, frames)
                assert 0 < want == int(dep.sum()) < dep.size, (case.name, where, at, "the framing gives", want, "the truth marks", int(dep.sum()))
                runs.append((f"{where}+Inf at {at}", poisoned, dep))
            for label, poisoned, dep in runs:
                rep.compare("B", label, view.fine, ctx, case.run(api, ctx, poisoned), y0, dep, strict)
            rep.compare("D", where + "after B", view.fine, ctx, case.run(api, ctx, ins), y0, np.zeros(dep.size, bool), False)
    finally:
        rep.print()
    rep.check()
