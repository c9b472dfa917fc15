"""No result depends on the order in which threads or workgroups run: the table of tests/amplitude_cases.py once more, and the core
plans beyond it, under every schedule of the CPU emulation (tests/emu/hipemu.h: Schedule).  Run by tests/test_schedule_emu.py; there
is no GPU twin -- on the device the order is the hardware's, and a test there passes or fails by timing.

Nothing of a case is restated: CASES, and each case's make, routes, select, unit_inputs, rounded, run, truth and bound, are
amplitude_cases'.  What is here: the schedules, the in-place placement, the core plan kinds the table does not hold, and the names
that are exempt.

Schedules.  The emulation runs the fibers of a block in ascending thread order between two barriers and hands the blocks out in
ascending order; its __shfl_xor is two whole-block barriers.  A hazard between a writer w and a reader r is then tried in one relative
order only, a reader workgroup never runs before its writer, and a missing __syncthreads() next to a shuffle is hidden.  HIPEMU_SCHEDULE
= "<threads>:<blocks>" (read at every launch) selects
  threads   ascending | descending | waves-descending (lanes ascending) | permutation-1 | permutation-2
  blocks    ascending (one worker per core) | descending | permutation (the last two on one worker, in exactly that order)
and under every schedule but the default a wave passes a shuffle when its own 64 lanes have arrived and runs on to its next block
barrier before the next wave starts.  SCHEDULES is every combination but the default: 14.

Checks.  Every comparison is bit for bit (amplitude_cases.differing == 0 over the whole output); there is no tolerance in this file.
  1  the handle table: per case, precision and route, y0 = case.run under the default schedule is held to the case's truth and bound
     once; the same call under each of SCHEDULES gives y0.
  2  in place, wherever include/fourier.h allows d_in == d_out (IN_PLACE: the core plan, fourier_hip_conv_*, fourier_hip_convnd_* with
     in_shape == out_shape == S, fourier_hip_r2r_*, the Hilbert envelope, the delay with C == 1, the cepstrum with m == n, the
     strided axis -- an N-D transform is one axis call out of place and then axis calls in place): InPlace hands the case's own run the
     output's address for its first input, which it has copied there.  The in-place result under the default schedule is y0, and so
     is the in-place result under each of SCHEDULES.
  3  the core beyond the table (KINDS): one length of every plan kind Plan::describe() names in the emulation -- the shortest that
     takes the route, asserted through describe() --, batch 3, the five transform codes, out of place and in place, as 1 and 2.  And
     every register-stage row the emulation build holds and every row of the tile cover tables of tests/golden/table_cover.json
     (tests/kernel_tables.py), forward and square-root-scaled inverse (between them both values of the kernels' `swap` and `scale`).
  4  WAITS_ON_OTHER_WORKGROUPS names, by the word describe() shows, the kernels that wait on other workgroups.  Such a kernel cannot
     finish under a serial block order (the workgroup it waits for has not started); it is left out of the schedules whose block
     order is not "ascending", and of nothing else.  The list may hold only kernels with an inter-workgroup wait.

What the schedules can show: a pairwise hazard whose two orders are both among them and whose stale value differs from the fresh one.
What they cannot: anything the memory model decides (a missing wait or fence), and every interleaving finer than a whole fiber run
between two yields.

A test prints one line -- the case, how many (route, schedule) runs were compared and how many reals differed -- then asserts."""
import contextlib
import math
import os
import re

import numpy as np

import amplitude_cases as cases
import kernel_tables as kt
from helpers import regfft_shape, rel_l2

ENV = "HIPEMU_SCHEDULE"
THREADS = ("ascending", "descending", "waves-descending", "permutation-1", "permutation-2")
BLOCKS = ("ascending", "descending", "permutation")
SCHEDULES = tuple((t, b) for t in THREADS for b in BLOCKS)[1:]
assert len(SCHEDULES) == 14 and ("ascending", "ascending") not in SCHEDULES

# describe() word -> why the kernel cannot run its blocks one after the other
WAITS_ON_OTHER_WORKGROUPS = {
    "xcd-l2": "fft_l2fused_kernel (plan option l2_fused, experiments build): persistent workgroups take (transform, pass, tile) items "
              "from the queue of their XCD and wait on counters that the workgroups of the pass before raise",
}

# families whose entry point allows d_in == d_out, with the cases of the family it holds for (include/fourier.h)
IN_PLACE = {
    "fft": lambda name: True,
    "axis": lambda name: True,
    "fftconv": lambda name: True,
    "convnd": lambda name: True,                            # the table's in_shape == out_shape == S
    "r2r": lambda name: True,
    "hilbert": lambda name: name.startswith("hilbert envelope"),   # analytic: the output is twice the input
    "delay": lambda name: " C=1 " in name,                  # any overlap is refused when C > 1
    "cepstrum": lambda name: True,                          # the table's m == n
}


def family(case):
    return case.name.split()[0]


def in_place(case):
    return IN_PLACE.get(family(case), lambda name: False)(case.name)


@contextlib.contextmanager
def schedule(threads, blocks):
    before = os.environ.get(ENV)
    os.environ[ENV] = f"{threads}:{blocks}"
    try:
        yield
    finally:
        if before is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = before


def exempt(d, sched):
    """the names of WAITS_ON_OTHER_WORKGROUPS that keep a plan described as d out of this schedule"""
    return [] if sched[1] == "ascending" else [word for word in WAITS_ON_OTHER_WORKGROUPS if word in d]


class InPlace:
    """the adapter with the output in the place of the first input: run() has the first array put() since the last run copied into
    the guarded output (the adapter's run(..., fill=)) and ptr() of that array is the output's address while the call runs.  The array must have the output's type and
    size, and the call must have asked for its address: a case that is not in place after all fails here."""

    def __init__(self, api):
        self.api, self.fa, self.device = api, api.fa, api.device
        self.first, self.alias, self.asked = None, None, 0

    def put(self, a):
        b = self.api.put(a)
        if self.first is None:
            self.first = (a, b)
        return b

    def ptr(self, b):
        if self.alias is not None and b is self.alias[0]:
            self.asked += 1
            return self.alias[1]
        return self.api.ptr(b)

    def run(self, call, shape, dtype):
        a, b = self.first
        assert a.dtype == np.dtype(dtype) and a.size == int(np.prod(shape)), ("not an in-place call", a.dtype, a.shape, dtype, shape)

        def aliased(out):
            self.alias, self.asked = (b, out), 0
            try:
                call(out)
            finally:
                self.alias = None
            assert self.asked == 1, ("the call asked for its input's address", self.asked, "times")

        return self.api.run(aliased, shape, dtype, fill=b)


def run_in_place(api, case, ctx, ins):
    """(a case that runs several calls -- convnd: correlate off and on -- puts its inputs once and runs twice: each in place)"""
    return case.run(InPlace(api), ctx, ins)


class HostApi(cases.HostApi):
    """amplitude_cases' adapter of the emulation build; run() can start from an output that holds `fill` (InPlace) instead of NaN"""

    def run(self, call, shape, dtype, fill=None):
        count = int(np.prod(shape))
        buf = np.full(count + 2 * cases.GUARD, cases.SENTINEL, dtype)
        out = buf[cases.GUARD:cases.GUARD + count]
        out[:] = np.nan if fill is None else fill.ravel()
        call(out.ctypes.data)
        assert np.all(buf[:cases.GUARD] == cases.SENTINEL) and np.all(buf[-cases.GUARD:] == cases.SENTINEL), "a guard element was written"
        return out.reshape(shape).copy()


class Report:
    """the figures of one test: ONE line, then everything is asserted"""

    def __init__(self, what):
        self.what, self.routes, self.failed = what, [], []
        self.runs = self.reals = self.left_out = 0
        self.worst = (0.0, 0.0, 1.0, "")

    def route(self, d):
        self.routes.append(d if not self.routes else d.split(":")[0].split(",")[0])

    def figure(self, where, value, bound):
        ratio = value / bound if value == value else math.inf
        if ratio >= self.worst[0]:
            self.worst = (ratio, value, bound, where)
        if not value <= bound:
            self.failed.append((where, value, bound))

    def same(self, where, y, y0):
        bad = cases.differing(y, y0)
        self.runs, self.reals = self.runs + 1, self.reals + bad
        if bad:
            self.failed.append((where, f"{bad} of {y0.size * (2 if y0.dtype.kind == 'c' else 1)} reals differ from the default schedule's"))

    def print(self):
        print(f"schedule {self.what}: {self.runs} (route, schedule) runs compared, {self.left_out} left out by name, {self.reals} reals differ; "
              f"default schedule: worst error {self.worst[1]:.3g} of {self.worst[2]:.3g} ({self.worst[3]})  [{' | '.join(self.routes)}]")

    def check(self):
        assert not self.failed, (self.what, self.failed)


def under_every_schedule(rep, where, d, run, y0, schedules=SCHEDULES):
    for sched in schedules:
        if exempt(d, sched):
            rep.left_out += 1
            continue
        with schedule(*sched):
            y = run()
        rep.same(f"{where}{sched[0]}:{sched[1]}", y, y0)


def table_runs(case, real):
    """the (route, schedule) runs check 1 compares for this case: nothing of the table is exempt"""
    return len(case.routes(real)) * len(SCHEDULES)


def check_table(api, case, real):
    """1, and 2 for the cases of IN_PLACE"""
    assert ENV not in os.environ, "the default schedule is the one without the variable"
    ctx = case.make(api, real)
    ins = cases.rounded(case.unit_inputs(ctx), real)
    case.conditions(ctx, ins)
    case.hold(ctx, ins)
    rep = Report(f"{real} {case.name}" + (", and in place" if in_place(case) else ""))
    try:
        for options, prefix in case.routes(real):
            where = cases.opt(options)
            d = case.select(ctx, real, options, prefix)
            rep.route(d)
            assert not exempt(d, ("ascending", "descending")), (case.name, d, "the table holds no kernel that waits on other workgroups")
            y0 = case.run(api, ctx, ins)
            rep.figure(f"{where}default", case.err(ctx, case.pick(ctx, y0), case.truth(ctx, ins)), case.bound(ctx, d, real))
            under_every_schedule(rep, where, d, lambda: case.run(api, ctx, ins), y0)
            if in_place(case):
                rep.same(f"{where}in place, default", run_in_place(api, case, ctx, ins), y0)
                under_every_schedule(rep, f"{where}in place, ", d, lambda: run_in_place(api, case, ctx, ins), y0)
        assert rep.runs == table_runs(case, real) * (2 if in_place(case) else 1) + (len(case.routes(real)) if in_place(case) else 0)
    finally:
        rep.print()
    rep.check()


# ---- 3: the core beyond the table
CODES = (0, 1, 2, 3, 4)  # fourier_amd.Transform
FFT, SQRT_SCALED_IFFT = 0, 4


def core_truth(x, code):
    wide, n = x.astype(np.complex128), x.shape[-1]
    if code in (0, 3):
        return np.fft.fft(wide, axis=-1) * (1.0 if code == 0 else 1.0 / math.sqrt(n))
    return np.fft.ifft(wide, axis=-1) * {1: 1.0, 2: float(n), 4: math.sqrt(n)}[code]


class Kind:
    """name; n: the length by precision; describe: what describe() must show (a prefix or a compiled pattern); env: the experiments
    build's switches, set while the plan is created; options: plan options, set after; codes: the transform codes (all five unless the
    length makes 150 runs a matter of minutes)"""

    def __init__(self, name, n, describe, env=None, options=None, codes=CODES):
        self.name, self.describe, self.env, self.options, self.codes = name, describe, env or {}, options or {}, codes
        self.n = n if isinstance(n, dict) else {"f32": n, "f64": n}


TWO_PASSES = {"f32": 1 << 16, "f64": 1 << 15}  # amplitude_cases.smallest_two_passes; asserted through describe() below
KINDS = [
    Kind("tiny, one 16-byte unit", 2, "stockham tiny(2) "),
    Kind("tiny, the most shuffle rounds", 16, "stockham tiny(16) "),
    Kind("whole rows", 64, "stockham 64 "),
    Kind("LDS mixed-radix", 6, "stockham mixed-radix 3.2 "),
    Kind("LDS mixed-radix, the kernel with run-time parameters", 54, "stockham mixed-radix ", env={"FOURIER_MIX_GENERIC": "1"}),
    Kind("register stages, two", 77, "stockham registers 11x7 one-launch "),
    Kind("register stages, three", 1001, "stockham registers 13x11x7 one-launch "),
    Kind("register stages on request", 729, "stockham registers 27x27 one-launch ", options={"register_stages": 1}),
    Kind("without the register stages", 1001, "stockham mixed-radix ", env={"FOURIER_NO_REGFFT": "1"}),
    Kind("one-launch power of two", {"f32": 2048, "f64": 1024}, re.compile(r"stockham \d+x\d+ one-launch ")),
    Kind("the one-launch size in two launches", 4096, cases.TWO_PASSES, env={"FOURIER_NO_TWOLEVEL": "1"}),
    Kind("two tile passes", TWO_PASSES, cases.TWO_PASSES),
    Kind("mixed tiles", 12288, "stockham mixed tiles 128x96 "),
    Kind("mixed tiles on the LDS tile kernels", {"f32": 20736, "f64": 13122}, "stockham mixed tiles ", env={"FOURIER_NO_REGTILE": "1"}),
    Kind("an odd pass behind the power-of-two passes", 3 * 4096, "stockham 64x64x3 ", env={"FOURIER_POW2_TILES_FIRST": "1"}),
    Kind("one global pass per radix", {"f32": 59049, "f64": 10368}, re.compile(r"stockham .*global-pass"), env={"FOURIER_NO_TILED_MIXED": "1"}),
    Kind("bluestein in one launch on register stages", 17, "bluestein M=36 registers 6x6 one-launch "),
    Kind("bluestein in one launch, fused", 1013, "bluestein M=2048 inner 64x32 one-launch fused "),
    Kind("bluestein in one launch, separate chirp sweeps", 1013, "bluestein M=2048 ", options={"bluestein_fusion": 0}),
    Kind("bluestein fused passes with the conv pass", {"f32": 20002, "f64": 10001}, re.compile(r"bluestein M=\d+ inner \d+x\d+ "),
         options={"bluestein_smooth_m": 0}),
    Kind("bluestein fused passes without the conv pass", {"f32": 20002, "f64": 10001}, re.compile(r"bluestein M=\d+ inner \d+x\d+ "),
         options={"bluestein_smooth_m": 0, "bluestein_conv": 0}),
    Kind("bluestein separate sweeps around the passes", {"f32": 20002, "f64": 10001}, re.compile(r"bluestein M=\d+ inner \d+x\d+ "),
         options={"bluestein_smooth_m": 0, "bluestein_fusion": 0}),
    Kind("bluestein chirp computed in the first pass", 40001, re.compile(r"bluestein M=131072 inner \d+x\d+ "),
         options={"bluestein_smooth_m": 0, "bluestein_chirp_compute": 1}, codes=(FFT, SQRT_SCALED_IFFT)),
    Kind("bluestein on a smooth work array", {"f32": 16411, "f64": 10007}, re.compile(r"bluestein M=\d+ inner mixed tiles \d+x\d+ ")),
    Kind("XCD-fused one launch", {"f32": 1 << 16, "f64": 1 << 15}, re.compile(r".*xcd-l2"), options={"l2_fused": 1}, codes=(FFT, SQRT_SCALED_IFFT)),
]
KIND_BY_NAME = {k.name: k for k in KINDS}
assert len(KIND_BY_NAME) == len(KINDS)

BATCH = 3


@contextlib.contextmanager
def environment(env):
    before = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for key, value in before.items():
            if value is None:
                del os.environ[key]
            else:
                os.environ[key] = value


def make_plan(api, n, real, env=None, options=None):
    with environment(env or {}):
        plan = api.fa.Fft(n, real, api.device)
    for key, value in (options or {}).items():
        plan.set_option(key, value)
    return plan


def core_inputs(n, real, seed, batch=BATCH):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(cases.cgauss(rng, batch, n).astype(cases.cdt(real)))


def core_runs(api, plan, x, code):
    """(out of place, in place) as closures that run the call once more"""
    def out_of_place():
        a = api
        dx = a.put(x)
        return a.run(lambda out: plan.transform_batch_ptr(a.ptr(dx), out, x.shape[0], code), x.shape, x.dtype)

    def in_place():
        a = InPlace(api)
        dx = a.put(x)
        return a.run(lambda out: plan.transform_batch_ptr(a.ptr(dx), out, x.shape[0], code), x.shape, x.dtype)

    return out_of_place, in_place


def check_plan(api, rep, plan, d, x, codes, real, schedules=SCHEDULES):
    """1 and 2 for one core plan: every code, out of place and in place, under every schedule"""
    for code in codes:
        out_of_place, placed = core_runs(api, plan, x, code)
        y0 = out_of_place()
        rep.figure(f"n={x.shape[-1]} code {code}", rel_l2(y0, core_truth(x, code)), cases.base_tol(d, real))
        rep.same(f"n={x.shape[-1]} code {code} in place, default", placed(), y0)
        under_every_schedule(rep, f"n={x.shape[-1]} code {code} ", d, out_of_place, y0, schedules)
        under_every_schedule(rep, f"n={x.shape[-1]} code {code} in place, ", d, placed, y0, schedules)


def check_kind(api, kind, real):
    assert ENV not in os.environ
    n = kind.n[real]
    if "register_stages" in kind.options:
        assert regfft_shape(n, cases.cdt(real), emu=True, on_request=True) is not None, (n, real)
    plan = make_plan(api, n, real, kind.env, kind.options)
    d = plan.describe()
    assert d.startswith(kind.describe) if isinstance(kind.describe, str) else kind.describe.match(d), (kind.name, real, d)
    rep = Report(f"{real} core, {kind.name}: n = {n}, codes {kind.codes}")
    rep.route(d)
    try:
        check_plan(api, rep, plan, d, core_inputs(n, real, n), kind.codes, real)
        left = len(kind.codes) * 2 * sum(1 for s in SCHEDULES if exempt(d, s))
        assert rep.left_out == left and rep.runs == len(kind.codes) * (2 * len(SCHEDULES) + 1) - left, (rep.runs, rep.left_out)
    finally:
        rep.print()
    rep.check()


# the ahead-of-time tables: every register-stage row the emulation build holds, and the rows of the tile cover tables
def emu_register_rows(real):
    return [r for r in kt.regfft_rows() if r.emu and not r.on_request and kt.flag(r, real)]


def cover_rows(key, real):
    return [(n, desc) for n, r, desc in kt.load_cover()[key] if r == real]


# The cover tables are 373 + 79 rows of up to 1.9 million points, 106 million in all: at batch 3 under 14 schedules twenty minutes of
# emulation.  Their rows run ONE transform under the two schedules that between them try every pair of threads, every pair of waves
# and every pair of blocks in the order the default does not, and a permutation of each -- what a tile pass can get wrong between
# two tiles of one transform does not need a second transform.  Every plan KIND above runs all 14 at batch 3.
COVER_PARTS = {"plain": 24, "blu": 4}  # a parametrised case holds every COVER_PARTS-th row of its cover table: a few seconds each
COVER_SCHEDULES = (("descending", "descending"), ("permutation-1", "permutation"))
assert set(COVER_SCHEDULES) <= set(SCHEDULES)


def check_rows(api, real, what, rows, batch=BATCH, schedules=SCHEDULES):
    """rows: (n, what describe() must hold)"""
    assert ENV not in os.environ
    rep = Report(f"{real} core, {what}: {len(rows)} lengths, batch {batch}, codes {(FFT, SQRT_SCALED_IFFT)}, {len(schedules)} schedules")
    try:
        for n, must in rows:
            plan = make_plan(api, n, real)
            d = plan.describe()
            assert must in d, (n, real, must, d)
            if not rep.routes:
                rep.route(d)
            check_plan(api, rep, plan, d, core_inputs(n, real, n, batch), (FFT, SQRT_SCALED_IFFT), real, schedules)
        assert rep.runs == len(rows) * 2 * (2 * len(schedules) + 1) and rep.left_out == 0
    finally:
        rep.print()
    rep.check()
