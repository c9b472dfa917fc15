"""No result depends on what the handle did before: the table of tests/amplitude_cases.py once more, stated once and run twice -- on
the CPU emulation (tests/test_history_emu.py) and on the MI355X (tests/test_gpu_history.py).  A handle owns scratch, pad regions,
tables, a window, chunk-walk parameters; every other test creates a handle, sets its state once and calls it with one batch and one
length.  A pad region zeroed at the first call only, a scratch sized by the first batch or a frame count kept from the first length
passes all of them.  The functional layer reuses cached handles, so a call history is the product's normal regime.

Nothing of a case is restated: CASES, and each case's make, routes, select, inputs, conditions, run, truth, err and bound, are
amplitude_cases'.  A case states its batch -- and a frame handle its length and frame count -- through its context (ctx.batch,
amplitude_cases.restate), so a caller can state them per call.  What is here: which cases share a handle, and the sequence.

Groups.  The cases that one handle serves form a group (GROUPS: by the first word of the case's name, exactly one rule per case --
group_of asserts it -- and the part of the name that states the constructor).  The members of a group are calls that differ in what the
ABI lets a CALL choose: the transform code of the core; forward and inverse of the real, N-D, STFT and MDCT handles; the r2r kind;
analytic signal and envelope; power 2, magnitude (normalised) and Welch; cross spectrum and coherence; the band spectrogram's power and
its logarithm with an active floor, then without; the plain and the PHAT weighting; NUFFT type 1 after type 2 with both signs and mode
orders; the cepstrum's log_mult.

The sequence.  ONE handle per group and precision goes through CALLS = 12 calls.  Call i is made
  by member     (i + i // 6) mod the group's size
  on route      (i // 2) mod the member's routes: every route option ("fusion", "weighting", "table", "accuracy") goes there and back
  with batch    3, 1, 7, 0, 9, 2, ...: it grows after it shrinks; 0 is a successful no-op that leaves the guarded output untouched
  with length   (frame handles) the table's, a shorter one, the shortest the handle takes (its fewest frames), one longer than
                anything before, the table's again, ...
  with window   (handles with set_window: STFT, MDCT, the spectrograms, cross spectrum, resampling) the table's, another, none (the
                handle's own: ones, the MDCT's sine window)
  with filters  (the convolutions, whose set_filters runs before every apply) 2, 1, 3, ... filters: fewer, then more; fftconv also with
                33, 17 and 9 taps; convnd sets the bank twice a call, `correlate` off and on
and `reserve` is called before call 5 at batch 2 (and the shortest length) and before call 8 at batch 8 and the longest length: the
batch 9 of call 10 lies beyond every earlier reserve.  Inputs are fresh Gaussians per call (seeded by name and call); a family that
states conditions on its inputs (PHAT, cepstrum) takes the first seed that meets them.

The check.  The output of call i is BIT-equal (amplitude_cases.differing == 0) to the output of a handle created for that call alone
and given only that call's state: same member, route, batch, length, window, filters.  The fresh handle's result is held to the member's f64
truth under the member's bound, so every compared value is anchored to the reference.  There is no tolerance in this file.

  with more     (STATES, per handle) the r2r norm ortho, backward, forward; `normalized` of the STFT and MDCT calls off and on;
                set_bands with the table's bank and two whose rows are shorter; nufft set_points with the table's points, the first
                half of them, all of them; the delays' values (like the weights: fresh per call); the core plan's route options
                "bluestein_fusion", "bluestein_conv" and "register_stages" -- those the plan takes -- there and back
                `correlate` of the 1-D convolutions off and on; `onesided_fold` and `scale` of the Welch and cross-spectrum calls;
                the N-D convolution's set_window through circular, full, same and valid, and its `filter_first` 0, 1, 3
Not varied here: the inner count of the axis case.

The f32 inner transforms' last bits depend on a row's parity within its launch (the cross-correlation and
non-uniform FFT handles under odd scratch bounds).  A reserve enlarges the history handle's scratch and could move its chunk walk away
from the fresh handle's; the batches here (at most 9 rows) stay inside one chunk on both, which the check would show otherwise."""
import collections
import re

import numpy as np

import amplitude_cases as cases
import mdct_truth

CALLS = 12
BATCHES = (3, 1, 7, 0, 9, 2)
WINDOWS = (0, 0, 0, 1, 1, 2, 2, 0, 1, 0, 2, 0)   # 0 the table's, 1 another, 2 none (ones)
FILTERS = (2, 2, 1, 1, 3, 3, 2, 1, 3, 3, 1, 2)   # set_filters: the table's count, fewer, more
TAPS = (33, 33, 33, 17, 17, 33, 9, 9, 33, 17, 33, 33)  # fftconv: the table's taps, shorter ones
RESERVES = {5: "small", 8: "large"}
RESERVED_BATCH = {"small": 2, "large": 8}
assert CALLS >= 8 and max(BATCHES) > max(RESERVED_BATCH.values()) and len(WINDOWS) == len(FILTERS) == len(TAPS) == CALLS
assert FILTERS[0] == cases.FILTERS and TAPS[0] == cases.TAPS

# family (first word) -> (group prefix, pattern of the part of the name that states the constructor)
Rule = collections.namedtuple("Rule", "families handle key frames")
GROUPS = (
    Rule(("fft",), "core", r"fft (\S+|smallest two passes) ", False),
    Rule(("rfft", "irfft"), "real", r"i?rfft (\d+)", False),
    Rule(("rfftn", "irfftn"), "realnd", r"i?rfftn (\[.*\])", False),
    Rule(("axis",), "axis", r"axis (\[.*\])", False),
    Rule(("r2r",), "r2r", r"r2r (\d+) ", False),
    Rule(("fftconv",), "fftconv", r"fftconv (\d+ \w+) ", False),
    Rule(("lconv",), "lconv", r"lconv (.* (?:real|complex)) ", False),
    Rule(("stft", "istft"), "stft", r"i?stft (.*)", True),
    Rule(("mdct", "imdct"), "mdct", r"i?mdct (\d+)", True),
    Rule(("pfb",), "pfb", r"pfb (.*)", True),
    Rule(("ipfb",), "ipfb", r"ipfb (.*)", True),
    Rule(("resample",), "resample", r"resample (.*)", False),
    Rule(("czt",), "czt", r"czt (.*)", False),
    Rule(("hilbert",), "hilbert", r"hilbert \w+ (\d+)", False),
    Rule(("spectrogram", "welch"), "spectrogram", r"\w+ (\d+ hop \d+)", True),
    Rule(("csd", "coherence"), "cross spectrum", r"\w+ (\d+ hop \d+)", True),
    Rule(("bandspec",), "bandspec", r"bandspec (\d+ \d+ bands)", True),
    Rule(("xcorr", "gcc-phat"), "xcorr", r"\S+ (\d+ n=\d+ \w+(?: composed)?) ", False),
    Rule(("delay",), "delay", r"delay (.* C=\d+) ", False),
    Rule(("convnd",), "convnd", r"convnd (\[.*\])", False),
    Rule(("nufft",), "nufft", r"nufft type \d (N=\d+ \S+)", False),
    Rule(("cepstrum",), "cepstrum", r"cepstrum (\d+ n=\d+ [\w\- ]+?) log_mult", False),
)


def family(case):
    return case.name.split()[0]


def group_of(case):
    found = [r for r in GROUPS if family(case) in r.families]
    assert len(found) == 1, (case.name, "is matched by", len(found), "group rules")
    m = re.match(found[0].key, case.name)
    assert m, (case.name, found[0].key)
    return found[0], f"{found[0].handle} {m.group(1)}"


def groups():
    out = collections.OrderedDict()
    for case in cases.CASES:
        rule, name = group_of(case)
        out.setdefault(name, (rule, []))[1].append(case)
    return out


GROUP = groups()
NAMES = list(GROUP)

# The groups whose header text allows a call to be captured into a graph (include/fourier.h, fourier_hip_transform_batch_*: "after a
# reserve the call never allocates and can be captured into a HIP graph").  CAPTURE_AT: the call before which the GPU twin reserves
# for the largest batch of the sequence, in and out of place, and captures; a buffer the plan owns only ever grows (DeviceBuffer::
# ensure), so no later call of the sequence moves what the graph points at -- tests/test_history_emu.py counts the allocations.
# Likewise the delay handle (fourier_hip_delay_*: "a captured graph may be replayed after [the delays and weights] were overwritten").
# Those are the header's only two statements about capture; no other family's text allows it, so no other family is captured here.
CAPTURABLE = tuple(name for name, (rule, members) in GROUP.items() if rule.handle in ("core", "delay"))
CAPTURE_AT = CALLS // 2


def reserve_for_capture(ctx, rule):
    """reserve for the largest batch of the sequence on every route the sequence takes: the core plan in and out of place, the delay
    handle on its composed route (the one-launch route owns nothing) -- and the route options as the call's state has them"""
    if rule.handle == "core":
        for in_place in (False, True):
            ctx.plan.reserve(max(BATCHES), in_place)
    else:
        ctx.plan.set_option("fusion", 0)
        ctx.plan.reserve(max(BATCHES) * ctx.plan.channels())
        for key, value in ctx.options.items():
            ctx.plan.set_option(key, value)


def freeze_options(i, ctx):
    """from the state of call CAPTURE_AT on the graph tests keep the core plan's options as created (state_core)"""
    ctx.captured = i >= CAPTURE_AT


# ---- the state of a call
def plans_of(ctx):
    return ctx.plan.plans if isinstance(ctx.plan, cases.Plans) else [ctx.plan]


def takes(ctx, fam, length):
    """(length, frames) the handle takes for this target: ipfb states frames and gives the length, the others the other way round"""
    if fam == "ipfb":
        return ctx.plan.length(length), length
    return length, ctx.plan.frames(length)


def lengths_of(ctx, fam):
    """the table's, a shorter one, the shortest the handle takes, one longer than anything before, the table's again -- as targets
    (ipfb: frame counts), each moved up to the next one the handle takes"""
    first = ctx.nf if fam == "ipfb" else ctx.length

    def valid_from(at):
        for v in range(max(1, at), 4 * first + 64):
            length, nf = takes(ctx, fam, v)  # (frames() is 0 where the handle does not take the length)
            if nf > 0 and length > 0:
                return v
        raise AssertionError((fam, at, "no valid length"))

    out = (first, valid_from(first // 2 + 1), valid_from(1), valid_from(2 * first + 7), first)
    assert out[2] <= out[1] < first < out[3], out
    return out


def windows_of(ctx):
    """the table's window, another of the same kind (the table's reversed, times 0.75, plus 0.125: positive and not symmetric), none"""
    if not (hasattr(ctx, "w") and hasattr(ctx.plan, "set_window_ptr")):
        return None
    return (ctx.w, np.ascontiguousarray(0.75 * ctx.w[::-1] + 0.125).astype(ctx.w.dtype), None)


def set_window(api, ctx, windows, which):
    if windows is None:
        return
    w = windows[which]
    if w is None:  # the handle's own: ones, or the MDCT's sine window
        ctx.plan.set_window_ptr(None)
        n = windows[0].size
        ctx.w, ctx.dw = (mdct_truth.sine_window(n // 2, windows[0].dtype) if isinstance(ctx.plan, api.fa.Mdct) else np.ones_like(windows[0])), None
    else:
        ctx.w, ctx.dw = w, api.put(w)
        ctx.plan.set_window_ptr(api.ptr(ctx.dw))


def reserve(ctx, rule, batch, target):
    """reserve on every handle of the context; False where the family's library has no reserve entry point (asked of the library
    by the entry point's name, so that an error inside a reserve that exists is an error here)"""
    fam = rule.families[0]
    plans = plans_of(ctx)
    if not all(hasattr(p._L, f"{p._prefix}reserve_{p._suffix}") for p in plans):
        return False
    for p in plans:
        if rule.frames:
            p.reserve(target if fam == "ipfb" else takes(ctx, fam, target)[0], batch)
        else:
            p.reserve(batch)
    return True


def inputs_for(case, ctx, real, seed):
    """fresh unit-variance inputs for the context's batch and length; the first seed whose inputs meet the family's conditions"""
    last = None
    for attempt in range(32):
        ins = cases.rounded(case.inputs(ctx, np.random.default_rng([seed, attempt])), real)
        try:
            case.conditions(ctx, ins)
            return ins
        except AssertionError as e:
            last = e
    raise AssertionError((case.name, "no inputs meet the conditions", last))


# ---- what else a call's state is, per handle: applied to the history handle before every call and to the fresh handle of that call
R2R_NORMS = ("ortho", "backward", "forward")
BAND_EDGES = (8000.0, 4000.0, 2000.0)   # the table's bank, and two whose rows are shorter (fewer bins a band)
CORE_OPTIONS = (("bluestein_fusion", 1), ("bluestein_conv", 1), ("register_stages", 0))  # with the value a fresh plan has


def state_r2r(api, ctx, real, i):
    ctx.norm = R2R_NORMS[i % len(R2R_NORMS)]
    return f"norm {ctx.norm}"


def state_normalized(api, ctx, real, i):
    ctx.normalized = bool((i // 2) % 2)
    return f"normalized {int(ctx.normalized)}"


def state_bands(api, ctx, real, i):
    """set_bands again: another bank of as many bands, with shorter rows"""
    edge = BAND_EDGES[i % len(BAND_EDGES)]
    W = api.fa.mel_filterbank(ctx.plan.n_fft() // 2 + 1, 0.0, edge, ctx.plan.bands(), 16000.0, None, "htk")
    ctx.W = np.asarray(W).astype(cases.rdt(real)).astype(np.float64)
    ctx.plan.set_bands(ctx.W)
    return f"bands up to {edge:g} Hz"


def state_points(api, ctx, real, i):
    """set_points again: the table's points, the first half of them (fewer), all of them (more)"""
    if not hasattr(ctx, "all_points"):
        ctx.all_points = [x.copy() for x in ctx.xs]
    some = i % 3 == 1
    for j, plan in enumerate(ctx.plan.plans):
        ctx.xs[j] = ctx.all_points[j][:len(ctx.all_points[j]) // 2] if some else ctx.all_points[j]
        plan.set_points(ctx.xs[j])
    return f"{len(ctx.xs[0])} points"


def state_core(api, ctx, real, i):
    """the route options of the core plan that this plan takes, there and back: the value a fresh plan has, the other one, ..."""
    if not hasattr(ctx, "takes_options"):
        ctx.takes_options, created = [], ctx.plan.describe()
        for key, fresh in CORE_OPTIONS:
            try:  # the value that leaves the plan as it was created: the listed one, unless describe() says the other (a Bluestein
                # plan on register stages has "register_stages" on)
                ctx.plan.set_option(key, fresh ^ 1)
                other = ctx.plan.describe()
                ctx.plan.set_option(key, fresh)
                if ctx.plan.describe() != created and other == created:
                    fresh ^= 1
                    ctx.plan.set_option(key, fresh)
                assert ctx.plan.describe() == created, (key, created, ctx.plan.describe())
                ctx.takes_options.append((key, fresh))
            except api.fa.FourierError:  # this plan has no such route
                assert ctx.plan.describe() == created, (key, created, ctx.plan.describe())
    said = []
    for k, (key, fresh) in enumerate(ctx.takes_options):
        # (a captured graph points at the plan's tables and work array, and "bluestein_fusion" can rebuild them: from the capture on
        # the graph tests keep the options as created -- include/fourier.h: "Rebuilds the plan's tables now")
        value = fresh if getattr(ctx, "captured", False) else fresh ^ ((i >> (k + 1)) & 1)
        ctx.plan.set_option(key, value)
        said.append(f"{key}={value}")
    return " ".join(said)


def state_correlate(api, ctx, real, i):
    ctx.correlate = bool((i // 3) % 2)
    return f"correlate {int(ctx.correlate)}"


def state_fold_scale(api, ctx, real, i):
    """onesided_fold and scale of welch_ptr / csd_ptr (the other calls of the group take neither)"""
    ctx.fold, ctx.scale = i % 2 == 0, (0.37, 1.0, 2.5)[i % 3]
    return f"fold {int(ctx.fold)} scale {ctx.scale:g}"


def state_convnd(api, ctx, real, i):
    """set_window again: the circular default, then the windows of the three linear modes for items of a = S - k + 1 (full: all of S;
    same: a from (k - 1) // 2; valid: from k - 1, a - k + 1 long and at least one sample a dimension); and filter_first 0, 1, 3"""
    S = ctx.plan._shape
    k = tuple(min(3, n) for n in S)
    a = tuple(n - m + 1 for n, m in zip(S, k))
    zero = (0,) * len(S)
    ctx.window = ((S, zero, S),
                  (a, zero, S),
                  (a, tuple((m - 1) // 2 for m in k), a),
                  (a, tuple(m - 1 for m in k), tuple(max(n - m + 1, 1) for n, m in zip(a, k))))[i % 4]
    ctx.filter_first = (0, 1, 3)[i % 3]
    return f"window {('circular', 'full', 'same', 'valid')[i % 4]}, filter_first {ctx.filter_first}"


STATES = {"fftconv": state_correlate, "lconv": state_correlate, "spectrogram": state_fold_scale, "cross spectrum": state_fold_scale,
          "convnd": state_convnd, "r2r": state_r2r, "stft": state_normalized, "mdct": state_normalized, "bandspec": state_bands, "nufft": state_points,
          "core": state_core}
assert set(STATES) <= {r.handle for r in GROUPS}


class Empty:
    """the adapter of an empty call: the output has the shape of ONE row's call (a NULL or dangling output is another matter: the
    entry points refuse it), the batch is 0 while the call runs"""

    def __init__(self, api, ctx):
        self.api, self.ctx, self.fa, self.device, self.put, self.ptr = api, ctx, api.fa, api.device, api.put, api.ptr

    def run(self, call, shape, dtype):
        def empty(out):
            self.ctx.batch = 0
            try:
                call(out)
            finally:
                self.ctx.batch = 1

        return self.api.run(empty, shape, dtype)


class Report:
    def __init__(self, what):
        self.what, self.failed, self.routes = what, [], []
        self.calls = self.compared = self.noops = self.reals = 0
        self.reserved = "no reserve entry point"
        self.worst = (0.0, 0.0, 1.0, "")

    def figure(self, where, value, bound):
        ratio = value / bound if value == value else float("inf")
        if ratio >= self.worst[0]:
            self.worst = (ratio, value, bound, where)
        if not value <= bound:
            self.failed.append((where, "the fresh handle against the truth", value, bound))

    def print(self):
        print(f"history {self.what}: {self.calls} calls, {self.compared} compared bit for bit with a fresh handle, {self.noops} empty; "
              f"{self.reals} reals differ; {self.reserved}; fresh handles: worst error {self.worst[1]:.3g} of {self.worst[2]:.3g} ({self.worst[3]})  "
              f"[{' | '.join(self.routes)}]")

    def check(self):
        assert not self.failed, (self.what, self.failed)


def state_of(i, members, real, lengths):
    case = members[(i + i // 6) % len(members)]
    routes = case.routes(real)
    return case, routes[(i // 2) % len(routes)], BATCHES[i % len(BATCHES)], (lengths[i % len(lengths)] if lengths else None), (WINDOWS[i], FILTERS[i], TAPS[i], i)


def apply_state(api, case, ctx, rule, real, route, batch, target, windows, which):
    """everything a call's state is, on this context; returns describe()"""
    ctx.batch = batch
    if target is not None:
        cases.restate(ctx, *takes(ctx, rule.families[0], target))
    set_window(api, ctx, windows, which[0])
    if hasattr(ctx, "filters"):  # the case's run sets them before it applies: fewer, then more filters, shorter taps
        ctx.filters = which[1]
    if hasattr(ctx, "taps"):
        ctx.taps = which[2]
    ctx.options = route[0]
    for key, fresh in getattr(ctx, "takes_options", ()):  # the table states the description of a plan with its options as created
        ctx.plan.set_option(key, fresh)
    d = case.select(ctx, real, *route)
    if rule.handle in STATES:  # (behind select: a core option may move the plan off the description the table states)
        ctx.said = STATES[rule.handle](api, ctx, real, which[3])
        d = case.describe(ctx)
    return d


def check_history(api, name, real, hooks=None):
    """the sequence on one handle.  hooks.before_state(i, ctx) is called before the state of call i is applied to that handle,
    hooks.before(i, ctx, case, ins) and hooks.after(i, ctx, case, ins, y) around the call (the graph capture of the GPU twin; the allocation count of the emulation)"""
    rule, members = GROUP[name]
    ctx = members[0].make(api, real)
    lengths = lengths_of(ctx, rule.families[0]) if rule.frames else None
    windows = windows_of(ctx)
    rep = Report(f"{real} {name} ({len(members)} table cases" + (f", lengths {lengths}" if lengths else "") + (", 3 windows" if windows else "") + ")")
    try:
        for i in range(CALLS):
            case, route, batch, target, which = state_of(i, members, real, lengths)
            if i in RESERVES:
                size = RESERVES[i]
                ok = reserve(ctx, rule, RESERVED_BATCH[size], (min(lengths) if size == "small" else max(lengths)) if lengths else None)
                rep.reserved = f"reserve before calls {sorted(RESERVES)}" if ok else rep.reserved
            if hooks is not None:
                hooks.before_state(i, ctx)
            where = f"call {i}: {case.name}, {cases.opt(route[0])}batch {batch}" + (f", length {target}" if lengths else "") + (f", window {which[0]}" if windows else "") + (f", {which[1]} filters" if hasattr(ctx, "filters") else "") + (f" of {which[2]} taps" if hasattr(ctx, "taps") else "")
            d = apply_state(api, case, ctx, rule, real, route, max(batch, 1), target, windows, which)
            if d.split(":")[0] not in rep.routes:
                rep.routes.append(d.split(":")[0])
            ins = inputs_for(case, ctx, real, sum(name.encode()) * 100 + i)  # (an empty call: one row, none of it read)
            if rule.handle == "delay":  # the device-resident delays change from call to call, like the weights: any finite value is valid
                ins[1] = np.random.default_rng(i).uniform(-9.5, 9.5, ins[1].shape).astype(ins[1].dtype)
            if getattr(ctx, "said", ""):
                where += ", " + ctx.said
            if hooks is not None:
                hooks.before(i, ctx, case, ins)
            y = case.run(api, ctx, ins) if batch else case.run(Empty(api, ctx), ctx, ins)
            if hooks is not None:
                hooks.after(i, ctx, case, ins, y)
            rep.calls += 1
            if batch == 0:  # between the guards nothing was written
                assert y.size and np.all(np.isnan(y)), (where, "an empty call wrote its output")
                rep.noops += 1
                continue
            fresh = case.make(api, real)
            fresh.captured = getattr(ctx, "captured", False)
            if hasattr(ctx, "takes_options"):  # the fresh handle gets the call's option values only, not the probe's round trips
                fresh.takes_options = ctx.takes_options
            assert apply_state(api, case, fresh, rule, real, route, batch, target, windows, which) == d, (where, "the fresh handle takes another route")
            case.conditions(fresh, ins)
            y1 = case.run(api, fresh, ins)
            rep.figure(where, case.err(fresh, case.pick(fresh, y1), case.truth(fresh, ins)), case.bound(fresh, d, real))
            bad = cases.differing(y, y1)
            rep.compared, rep.reals = rep.compared + 1, rep.reals + bad
            if bad:
                rep.failed.append((where, f"{bad} of {y.size * (2 if y.dtype.kind == 'c' else 1)} reals differ from the fresh handle's"))
        assert rep.calls == CALLS and rep.compared + rep.noops == CALLS
    finally:
        rep.print()
    rep.check()
