"""What a core plan runs is a function of the option values last set on it -- not of the order in which they were set, nor of values
set before them (include/fourier.h, "THE RULE").  Stated once and run twice: on the CPU emulation (tests/test_option_emu.py) and on
the MI355X (tests/test_gpu_options.py).  Every other test sets each option alone, once, on a fresh plan; the state behind the options
is hand-kept in Plan<T> (fourier_amd/csrc/plan.h), and a rebuild of the Bluestein route re-derives most of it.

Inputs are seeded Gaussians (helpers.hash_normal).  Truth, error and bound are those of the core `fft` cases of
tests/amplitude_cases.py (CORE_TRUTH, rel_l2, base_tol): no tolerance is introduced here.  Under "bluestein_reference_chirp" = 1 in
f64 the result is ALSO held to the oracle at the bound of test_engine_emu.py::test_bluestein_reference_chirp_option (REFERENCE_CHIRP_TOL).

The Bluestein matrix (check_bluestein).  BLUESTEIN lists the lengths with the route every value of "bluestein_smooth_m" gives, asserted
from describe() before anything relies on it.  The 48 states of smooth_m x fusion x conv x chirp_compute x reference_chirp are each
reached by four sequences of set_option on four fresh plans: canonical order; reversed; a seeded random order; canonical order after
every option was first set to its OTHER value.  Batch 3, the codes Fft and Ifft (scaled).  Per state:
  (i)   the non-empty profile slots, describe() and model_bytes() are equal across the four sequences
  (ii)  the outputs are bit-equal across the four sequences
  (iii) the canonical plan's output is within the bound of the f64 truth
  (iv)  plain and profiled, in place and out of place: four calls, bit-equal
  (v)   describe() does not say "fused" where the slots contain blu_pre
and over the 48 states of a length (check_bluestein_across_states, a test case of its own that runs each state's canonical plan once
more and so depends on no other case), with effective() -- the rule's precedence written out: what of a state the route does NOT ignore --
  (vi)  states with the same effective state have equal slots, describe(), model_bytes() AND bits
  (vii) states whose effective states differ differ in (slots, describe, model_bytes); where they differ in fused / separate or in
        conv / no-conv alone, in their slot lists; computed against read chirp in model_bytes (and in f32 in their bits); the
        reference's chirp against the exact one in their f64 bits.  This makes "every option ignored" fail.
SEQUENCES names the shortest orders that show three defects of hand-kept option state: an option undone by a later smooth_m, a
chirp_compute request lost across a rebuild of the route, a describe() left stale by fusion = 0.

The two-pass matrix (check_two_pass): "scratch" x "chunk_bytes" x "stream_pipeline" x "tile_walk" x "tile_walk_last" on f32 2^16 and
f64 2^15, batch 5 (a ragged last chunk).  In every state the four call kinds are bit-equal to a default plan's output (which is held
to the truth); after reserve(5, False) and reserve(5, True) none of them allocates (the emulation counts); "stream_pipeline" back to
0: the same bits; in the product library the experiments' options return INVALID_ARGUMENT and change nothing.

Every other route (check_other_route): "scratch" = 1 and "chunk_bytes" = one row, in both orders, change no bit of any call kind;
"register_stages" 1 -> 0 -> 1 interleaved with them gives the bits of a fresh plan with the final values."""
import collections
import itertools
import re

import numpy as np

import amplitude_cases as cases
from helpers import hash_normal, rel_l2

FFT, IFFT = cases.FFT, cases.IFFT
CODES = (FFT, IFFT)
REFERENCE_CHIRP_TOL = 5e-15

BLU_KEYS = ("bluestein_smooth_m", "bluestein_fusion", "bluestein_conv", "bluestein_chirp_compute", "bluestein_reference_chirp")
BLU_VALUES = ((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1))
BLU_STATES = tuple(itertools.product(*BLU_VALUES))
assert len(BLU_STATES) == 48

# the four ways to make one call: (name, profiled, in place)
KINDS = (("plain", False, False), ("plain in place", False, True), ("profiled", True, False), ("profiled in place", True, True))

ONE_LAUNCH = r"bluestein M=%d inner \S+( one-launch)? fused f"
REGISTERS = r"bluestein M=%d registers \S+ one-launch f"
TILES = r"bluestein M=%d inner mixed tiles %s f"
PASSES = r"bluestein M=%d inner %s f"
# length, precision, {smooth_m: the route of a fresh plan with that value alone}.  (Both twins run all 48 states at every length: the
# emulation is not thinned to a pairwise cover, a state takes it a fraction of a second.)
Blu = collections.namedtuple("Blu", "n real routes")
BLUESTEIN = (
    Blu(439, "f32", {0: ONE_LAUNCH % 1024, 1: ONE_LAUNCH % 1024, 2: REGISTERS % 900}),
    Blu(3001, "f32", {0: ONE_LAUNCH % 8192, 1: ONE_LAUNCH % 8192, 2: REGISTERS % 8820}),
    Blu(20002, "f32", {0: PASSES % (65536, "256x256"), 1: TILES % (40320, r"\d+x\d+"), 2: TILES % (40320, r"\d+x\d+")}),
    Blu(40001, "f32", {0: PASSES % (131072, "512x256"), 1: TILES % (81000, r"\d+x\d+"), 2: TILES % (81000, r"\d+x\d+")}),
    Blu(439, "f64", {0: ONE_LAUNCH % 1024, 1: REGISTERS % 900, 2: REGISTERS % 900}),
    Blu(10007, "f64", {0: PASSES % (32768, "256x128"), 1: TILES % (20160, "168x120"), 2: TILES % (20160, "168x120")}),
)
BLU_NAMES = [f"{b.n} {b.real}" for b in BLUESTEIN]
BLU_BY_NAME = dict(zip(BLU_NAMES, BLUESTEIN))


def inputs(n, real, batch, seed=0):
    return np.ascontiguousarray(np.stack([hash_normal(1000 * seed + n % 997 + b, n) for b in range(batch)]).astype(cases.cdt(real)))


def truth(x, code):
    return cases.CORE_TRUTH[code](x.astype(np.complex128))


def call(api, plan, x, code, profiled=False, in_place=False):
    """one call of `plan` on the rows of x, its output between guard elements; returns (output, non-empty profile slots)"""
    dx = None if in_place else api.put(x)
    slots = []

    def go(out):
        src = out if in_place else api.ptr(dx)
        if profiled:
            slots.extend(plan.profile_batch_ptr(src, out, x.shape[0], code))
        else:
            plan.transform_batch_ptr(src, out, x.shape[0], code)

    y = api.run(go, x.shape, x.dtype, fill=x if in_place else None)
    return y, tuple(s[0] for s in slots if s[2] > 0)


def make(api, n, real, settings=()):
    plan = api.fa.Fft(n, real, api.device)
    for key, value in settings:
        plan.set_option(key, value)
    return plan


class Report:
    def __init__(self, what):
        self.what, self.failed, self.calls, self.compared, self.routes = what, [], 0, 0, []
        self.worst = (0.0, 0.0, 1.0, "")

    def figure(self, where, value, bound):
        ratio = value / bound if value == value else float("inf")
        if ratio >= self.worst[0]:
            self.worst = (ratio, value, bound, where)
        if not value <= bound:
            self.failed.append((where, "against the truth", value, bound))

    def same(self, where, a, b):
        self.compared += 1
        if isinstance(a, np.ndarray):
            bad = cases.differing(a, b)
            if bad:
                self.failed.append((where, f"{bad} of {2 * a.size} reals differ"))
        elif a != b:
            self.failed.append((where, a, b))

    def differ(self, where, a, b):
        self.compared += 1
        if (cases.differing(a, b) == 0) if isinstance(a, np.ndarray) else (a == b):
            self.failed.append((where, "do not differ", a if not isinstance(a, np.ndarray) else ""))

    def route(self, d):
        if d not in self.routes:
            self.routes.append(d)

    def print(self):
        print(f"options {self.what}: {self.calls} calls, {self.compared} comparisons, {len(self.failed)} failed; worst error "
              f"{self.worst[1]:.3g} of {self.worst[2]:.3g} ({self.worst[3]})  [{' | '.join(self.routes)}]")

    def check(self):
        assert not self.failed, (self.what, len(self.failed), self.failed[:12])


# ---- the Bluestein matrix
def other(i, v):
    return (v + 1) % 3 if i == 0 else 1 - v


def sequences(state, seed):
    """the four sequences of (key, value) that end in `state`"""
    canon = list(zip(BLU_KEYS, state))
    order = list(np.random.default_rng(seed).permutation(len(canon)))
    while order in (sorted(order), sorted(order, reverse=True)):  # neither of the two orders already there
        order = order[1:] + order[:1]
    away = [(key, other(i, v)) for i, (key, v) in enumerate(canon)]
    return (("canonical", canon), ("reversed", canon[::-1]), ("random order", [canon[i] for i in order]), ("from the other values", away + canon))


def category(d):
    return "registers" if " registers " in d else "tiles" if " mixed tiles " in d else "one launch" if " fused f" in d else "passes"


def effective(routes, state):
    """The rule's precedence, written out: what of `state` the plan does not ignore, given the description routes[smooth_m] of a fresh
    plan with that "bluestein_smooth_m" alone.  (route, form, chirp source, tables)"""
    smooth_m, fusion, conv, compute, reference = state
    route = routes[smooth_m]
    if category(route) == "registers" and not fusion:  # the register route has no unfused form: the reference's power-of-two M
        route = routes[0]
    kind = category(route)
    if kind in ("registers", "tiles"):  # fusion (now 1, or ignored), conv and chirp_compute are ignored
        form, chirp = "", ""
    elif not fusion:  # conv needs fusion, and so does the computed chirp
        form, chirp = "separate", ""
    elif kind == "one launch":
        form, chirp = "fused", ""
    else:
        form, chirp = ("conv" if conv else "no-conv"), ("computed" if compute and not reference else "read")
    return (route, form, chirp, reference)


Seen = collections.namedtuple("Seen", "slots describe model y")


def observe(api, rep, plan, x, every_kind, where):
    """(iv) where every_kind; the forward call profiled for its slots, the inverse plain"""
    ys = []
    for code in CODES:
        y, slots = call(api, plan, x, code, profiled=(code == FFT))
        rep.calls += 1
        if code == FFT:
            named = slots
        if every_kind:
            for kind, profiled, in_place in KINDS:
                if (profiled, in_place) != (code == FFT, False):
                    rep.same(f"{where} code {code}: {kind} against {'profiled' if code == FFT else 'plain'}", call(api, plan, x, code, profiled, in_place)[0], y)
                    rep.calls += 1
        ys.append(y)
    return Seen(named, plan.describe(), plan.model_bytes(), tuple(ys))


def routes_of(api, blu):
    """before relying on the length: the route of each value of smooth_m, alone on a fresh plan, asserted against the table"""
    routes = {}
    for value, pattern in blu.routes.items():
        routes[value] = make(api, blu.n, blu.real, [("bluestein_smooth_m", value)]).describe()
        assert re.match(pattern, routes[value]), (blu.n, blu.real, value, routes[value], pattern)
    assert make(api, blu.n, blu.real).describe() == routes[1], (blu.n, blu.real, "the default is smooth_m = 1")
    return routes


def said_of(state):
    return " ".join(f"{k.replace('bluestein_', '')}={v}" for k, v in zip(BLU_KEYS, state))


def check_bluestein(api, oracle, name, smooth_m):
    """(i) ... (v) for the 16 states of one value of "bluestein_smooth_m" (a test case of a few seconds)"""
    blu = BLU_BY_NAME[name]
    n, real = blu.n, blu.real
    states = [s for s in BLU_STATES if s[0] == smooth_m]
    assert len(states) == 16
    rep = Report(f"bluestein {name}, smooth_m = {smooth_m}: {len(states)} states x 4 sequences")
    x = inputs(n, real, cases.BATCH)
    want = {code: truth(x, code) for code in CODES}
    reference = {code: oracle.transform_batch(x, code) for code in CODES} if real == "f64" else None
    routes_of(api, blu)
    try:
        for state in states:
            first = None
            for how, settings in sequences(state, [n, BLU_STATES.index(state)]):
                where = f"{said_of(state)} ({how})"
                got = observe(api, rep, make(api, n, real, settings), x, first is None, where)
                if first is None:
                    first = got
                    rep.route(got.describe)
                    for code, y in zip(CODES, got.y):  # (iii)
                        rep.figure(f"{where} code {code}", rel_l2(y, want[code]), cases.base_tol(got.describe, real))
                        if reference is not None and state[4] == 1:
                            rep.figure(f"{where} code {code} against the oracle", rel_l2(y, reference[code]), REFERENCE_CHIRP_TOL)
                    if "blu_pre" in got.slots:  # (v)
                        rep.same(f"{where}: describe() of a plan that runs blu_pre says fused", "fused" in got.describe, False)
                    continue
                for field in ("slots", "describe", "model"):  # (i)
                    rep.same(f"{where} against canonical: {field}", getattr(got, field), getattr(first, field))
                for code, a, b in zip(CODES, got.y, first.y):  # (ii)
                    rep.same(f"{where} against canonical: code {code}", a, b)
    finally:
        rep.print()
    rep.check()


def check_bluestein_across_states(api, name):
    """(vi) and (vii) for one length, in one test case of its own: the canonical plan of each of the 48 states once more, so that the
    comparisons across the values of smooth_m depend on no other test case having run, in this process or before this one"""
    blu = BLU_BY_NAME[name]
    n, real = blu.n, blu.real
    rep = Report(f"bluestein {name}, across the {len(BLU_STATES)} states")
    x = inputs(n, real, cases.BATCH)
    routes = routes_of(api, blu)
    try:
        seen = collections.OrderedDict((state, observe(api, rep, make(api, n, real, zip(BLU_KEYS, state)), x, False, said_of(state))) for state in BLU_STATES)
        by_effect = collections.OrderedDict()
        for state in seen:
            by_effect.setdefault(effective(routes, state), []).append(state)
        for effect, members in by_effect.items():  # (vi)
            rep.route(seen[members[0]].describe)
            for state in members[1:]:
                a, b = seen[members[0]], seen[state]
                for field in ("slots", "describe", "model"):
                    rep.same(f"{state} against {members[0]}, both {effect}: {field}", getattr(b, field), getattr(a, field))
                for code, ya, yb in zip(CODES, a.y, b.y):
                    rep.same(f"{state} against {members[0]}, both {effect}: code {code}", yb, ya)
        for (ea, ma), (eb, mb) in itertools.combinations(by_effect.items(), 2):  # (vii)
            a, b, where = seen[ma[0]], seen[mb[0]], f"{ma[0]} {ea} against {mb[0]} {eb}"
            if ea[:3] != eb[:3]:
                rep.differ(f"{where}: (slots, describe, model_bytes)", a[:3], b[:3])
            if ea[0] == eb[0] and ea[1] != eb[1]:  # fused against separate, conv against no-conv: other kernels
                rep.differ(f"{where}: slots", a.slots, b.slots)
            if ea[:2] == eb[:2] and ea[3] == eb[3] and ea[2] != eb[2]:  # the chirp computed or read
                rep.differ(f"{where}: model_bytes", a.model, b.model)
                if real == "f32":
                    rep.differ(f"{where}: bits", a.y[0], b.y[0])
            if ea[:3] == eb[:3] and ea[3] != eb[3]:  # the reference's chirp angle: the same kernels on other tables
                rep.same(f"{where}: slots", a.slots, b.slots)
                if real == "f64":
                    rep.differ(f"{where}: bits", a.y[0], b.y[0])
        rep.what += f": {len(by_effect)} effective states"
        assert len(by_effect) > len(set(routes.values())), (name, list(by_effect))  # the options tell states apart beyond smooth_m
    finally:
        rep.print()
    rep.check()


# Defects of hand-kept option state, each as the shortest order that shows it: an option undone by a later "bluestein_smooth_m", a
# "bluestein_chirp_compute" request lost across a rebuild of the route, a describe() left stale by "bluestein_fusion".  Each is held
# against a fresh plan that gets the final values once, in canonical order.  name -> lengths, sequence
SEQUENCES = collections.OrderedDict((
    ("conv off, then the power-of-two M", ((("10007 f64", "40001 f32", "20002 f32")), (("bluestein_conv", 0), ("bluestein_smooth_m", 0)))),
    ("fusion off, then the power-of-two M", ((("10007 f64", "40001 f32", "20002 f32")), (("bluestein_fusion", 0), ("bluestein_smooth_m", 0)))),
    ("fusion off, then every smooth M", ((("439 f32", "3001 f32")), (("bluestein_fusion", 0), ("bluestein_smooth_m", 2)))),
    ("every smooth M, then fusion off", ((("439 f32", "3001 f32")), (("bluestein_smooth_m", 2), ("bluestein_fusion", 0)))),
    ("a chirp_compute request across a rebuild", ((("40001 f32",)), (("bluestein_chirp_compute", 1), ("bluestein_reference_chirp", 1),
                                                                    ("bluestein_smooth_m", 0), ("bluestein_reference_chirp", 0)))),
    ("fusion off alone", ((("439 f32", "3001 f32")), (("bluestein_fusion", 0),))),
))
SEQUENCE_NAMES = [f"{name}: {length}" for name, (lengths, seq) in SEQUENCES.items() for length in lengths]


def check_sequence(api, which):
    name, length = which.rsplit(": ", 1)
    blu, settings = BLU_BY_NAME[length], SEQUENCES[name][1]
    rep = Report(f"sequence {which}")
    x = inputs(blu.n, blu.real, cases.BATCH)
    final = dict(settings)
    try:
        got = observe(api, rep, make(api, blu.n, blu.real, settings), x, False, "the sequence")
        fresh = observe(api, rep, make(api, blu.n, blu.real, [(k, final[k]) for k in BLU_KEYS if k in final]), x, False, "the final values")
        rep.route(fresh.describe)
        for field in ("slots", "describe", "model"):
            rep.same(field, getattr(got, field), getattr(fresh, field))
        for code, a, b in zip(CODES, got.y, fresh.y):
            rep.same(f"code {code}", a, b)
            rep.figure(f"code {code}", rel_l2(b, truth(x, code)), cases.base_tol(fresh.describe, blu.real))
        if "blu_pre" in got.slots:
            rep.same("describe() of a plan that runs blu_pre says fused", "fused" in got.describe, False)
        if final.get("bluestein_fusion") == 0:  # on these lengths' routes fusion = 0 is not ignored
            rep.same("fusion = 0 runs the separate sweeps", "blu_pre" in got.slots and "blu_post" in got.slots, True)
        if final.get("bluestein_conv") == 0:
            rep.same("conv = 0 runs no conv kernel", "conv_pass" in got.slots, False)
        if final.get("bluestein_chirp_compute") == 1:
            read = make(api, blu.n, blu.real, [(k, 0 if k == "bluestein_chirp_compute" else final[k]) for k in BLU_KEYS if k in final])
            rep.differ("model_bytes with the chirp read", got.model, read.model_bytes())
            rep.differ("bits with the chirp read", got.y[0], call(api, read, x, FFT)[0])
    finally:
        rep.print()
    rep.check()


# ---- the two-pass matrix
BATCH2 = 5
TWO_PASS = {"f32": (1 << 16, "stockham 256x256 f32"), "f64": (1 << 15, "stockham 256x128 f64")}
PIPELINES = (0, 2 | 2 << 16, 2 | 3 << 16 | 1 << 24)
TWO_KEYS = ("scratch", "chunk_bytes", "stream_pipeline", "tile_walk", "tile_walk_last")
EXPERIMENTS_ONLY = ("l2_fused", "last_pass_prefetch", "skeleton")
INVALID_ARGUMENT = 1  # FOURIER_HIP_INVALID_ARGUMENT, include/fourier.h


def two_pass_states(real):
    row = TWO_PASS[real][0] * np.dtype(cases.cdt(real)).itemsize
    return tuple(itertools.product((0, 1), (0, row, 2 * row), PIPELINES, (0, 4 | 1 << 8), (0, 8)))


def check_two_pass(api, real, states=None, alloc_count=None, product=False):
    """alloc_count() -> the allocations so far (the emulation's counter; None: not counted)"""
    n, described = TWO_PASS[real]
    states = two_pass_states(real) if states is None else states
    rep = Report(f"two passes {real} 2^{n.bit_length() - 1}, {len(states)} states")
    x = inputs(n, real, BATCH2)
    default = make(api, n, real)
    assert default.describe() == described, default.describe()
    default.set_option("stream_pipeline", PIPELINES[1])  # accepted on this plan ...
    default.set_option("stream_pipeline", 0)
    base = {code: call(api, default, x, code)[0] for code in CODES}
    rep.route(described)
    try:
        for code in CODES:
            rep.figure(f"default code {code}", rel_l2(base[code], truth(x, code)), cases.base_tol(described, real))
        for state in states:
            said = " ".join(f"{k}={v}" for k, v in zip(TWO_KEYS, state))
            plan = make(api, n, real, zip(TWO_KEYS, state))
            if product:
                for key in EXPERIMENTS_ONLY:  # (the entry point itself: the Python layer's FourierError does not carry the status)
                    rep.same(f"{said}: the status of {key} = 1 in the product library", plan._fn("set_option")(plan._h, key.encode(), 1), INVALID_ARGUMENT)
            rep.same(f"{said}: describe", plan.describe(), described)
            plan.reserve(BATCH2, False)
            plan.reserve(BATCH2, True)
            before = alloc_count() if alloc_count else 0
            for code in CODES:
                for kind, profiled, in_place in KINDS:
                    rep.same(f"{said}: code {code} {kind} against the default plan", call(api, plan, x, code, profiled, in_place)[0], base[code])
                    rep.calls += 1
            if alloc_count:
                rep.same(f"{said}: allocations after reserve({BATCH2}) out of and in place", alloc_count() - before, 0)
            plan.set_option("stream_pipeline", 0)
            for in_place in (False, True):
                rep.same(f"{said}, stream_pipeline back to 0{', in place' if in_place else ''}", call(api, plan, x, FFT, False, in_place)[0], base[FFT])
                rep.calls += 1
    finally:
        rep.print()
    rep.check()


# ---- every other route
OTHER_ROUTES = collections.OrderedDict((
    ("one launch", (4096, "stockham 64x64 one-launch ")),
    ("LDS mixed radix", (1000, "stockham mixed-radix 5.5.5.8 ")),
    ("register stages", (1001, "stockham registers 13x11x7 one-launch ")),
    ("ahead-of-time tile passes", (100000, "stockham mixed tiles 400x250 ")),
    ("global passes", ({"f32": 59049, "f64": 10368}, "stockham global-pass ")),
))
# No length up to 3 * 10^6 takes the global passes by default (every 2^a 3^b, a < 12, has a tile factorisation there): the route is
# reached as tests/test_engine_emu.py and tests/test_gpu_parity.py reach it, with GLOBAL_PASS_ENV in the environment, which the
# emulation and the experiments library honour (the product library reads no environment): the twins bind that library for this route.
GLOBAL_PASS_ENV = ("FOURIER_NO_TILED_MIXED", "1")
ON_REQUEST = 4608  # a 2^a 3^b length with a register-stage kernel listed on request in both precisions (include/fourier.h, "register_stages")


def check_other_route(api, which, real):
    n, prefix = OTHER_ROUTES[which]
    n = n[real] if isinstance(n, dict) else n
    row = n * np.dtype(cases.cdt(real)).itemsize
    rep = Report(f"{which} {n} {real}")
    x = inputs(n, real, cases.BATCH)
    default = make(api, n, real)
    described = default.describe()
    assert described.startswith(prefix), described
    rep.route(described)
    base = {code: call(api, default, x, code)[0] for code in CODES}
    try:
        for code in CODES:
            rep.figure(f"default code {code}", rel_l2(base[code], truth(x, code)), cases.base_tol(described, real))
        settings = (("scratch", 1), ("chunk_bytes", row))
        for order in (settings, settings[::-1]):
            plan = make(api, n, real, order)
            rep.same(f"{order}: describe", plan.describe(), described)
            for code in CODES:
                for kind, profiled, in_place in KINDS:
                    rep.same(f"{order}: code {code} {kind} against the default plan", call(api, plan, x, code, profiled, in_place)[0], base[code])
                    rep.calls += 1
    finally:
        rep.print()
    rep.check()


def check_register_stages_interleaved(api, real):
    """ "register_stages" 1 -> 0 -> 1 with "scratch" and "chunk_bytes" set in between: the bits of a fresh plan with the final values"""
    n = ON_REQUEST
    row = n * np.dtype(cases.cdt(real)).itemsize
    rep = Report(f"register_stages interleaved {n} {real}")
    x = inputs(n, real, cases.BATCH)
    for final in (1, 0):
        walk = [("register_stages", 1), ("scratch", 1), ("register_stages", 0), ("chunk_bytes", row), ("register_stages", 1)] + ([("register_stages", 0)] if final == 0 else [])
        plan = make(api, n, real, walk)
        fresh = make(api, n, real, [("scratch", 1), ("chunk_bytes", row), ("register_stages", final)])
        assert ("registers" in fresh.describe()) == (final == 1), fresh.describe()
        rep.route(fresh.describe())
        rep.same(f"final {final}: describe", plan.describe(), fresh.describe())
        for code in CODES:
            want = call(api, fresh, x, code)[0]
            rep.figure(f"final {final} code {code}", rel_l2(want, truth(x, code)), cases.base_tol(fresh.describe(), real))
            for kind, profiled, in_place in KINDS:
                rep.same(f"final {final}: code {code} {kind} against the fresh plan", call(api, plan, x, code, profiled, in_place)[0], want)
                rep.calls += 1
    rep.print()
    rep.check()
