"""No result depends on the handle's call history, on the MI355X: tests/history_cases.py through the product library.  The CPU twin
is tests/test_history_emu.py; the two run the same sequences and make the same assertion: every call of one handle that goes through
twelve calls of changing kind, route, batch, length and window gives, bit for bit, what a fresh handle gives for that call alone, and
the fresh handle's result is within the family's bound of the f64 truth.  Inputs on the device, every output pre-filled with NaN
between guard elements (tests/test_gpu_amplitude.py's DeviceApi).  What the emulation cannot say: the product's route tables and
chunk walks are not the emulator's, and a stale pad region or scratch row is only read by the kernels that exist here.

Two checks only the hardware can make.  The in-place calls of tests/schedule_cases.py at a batch whose smallest grid is, by a stated
lower estimate, four times the workgroups 256 compute units hold, bit-equal to the out-of-place call (which asserts nothing about
order: it widens the window).  And a call captured into a graph after half the sequence, replayed after the other half, gives the
bits of the eager call (the groups of history_cases.CAPTURABLE, whose header text allows capture; reserve first, then the capture, as
the other graph tests do)."""
import re

import numpy as np
import pytest

import amplitude_cases as cases
import history_cases as history
import schedule_cases as schedule
from test_gpu_amplitude import DeviceApi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def api(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    return DeviceApi(torch, fourier_amd)


def test_every_case_is_in_exactly_one_group():
    seen = [c.name for rule, members in history.GROUP.values() for c in members]
    assert sorted(seen) == sorted(cases.NAMES)


@pytest.mark.parametrize("name", history.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_a_call_gives_what_a_fresh_handle_gives(api, real, name):
    history.check_history(api, name, real)


class Captures:
    """before call CAPTURE_AT: reserve for the largest batch of the sequence, in and out of place (from here on no call of the
    sequence allocates: a plan-owned buffer only grows), one eager call on the capture stream, then the same call captured.  The
    sequence goes on with other kinds of call, batches and routes; replay() then runs the graph and the eager call side by side."""

    def __init__(self, torch, api, rule):
        self.torch, self.api, self.rule, self.graph = torch, api, rule, None

    def before_state(self, i, ctx):
        history.freeze_options(i, ctx)

    def before(self, i, ctx, case, ins):
        if i != history.CAPTURE_AT:
            return
        torch, plan = self.torch, ctx.plan
        assert ctx.batch > 0
        history.reserve_for_capture(ctx, self.rule)
        self.held = [self.api.put(a) for a in ins]  # the buffers the graph points at
        if self.rule.handle == "core":
            code = int(self.api.fa.Transform[case.name.split()[-1]])
            self.what = f"batch {ctx.batch}, code {code}"
            shape, dtype = ins[0].shape, self.held[0].dtype
            self.call = lambda out, stream: plan.transform_batch_ptr(self.held[0].data_ptr(), out.data_ptr(), ctx_batch, code, stream)
        else:  # the delay handle: rows, delays and weights, all on the device
            rows = ctx.batch * plan.channels()
            self.what = f"{rows} rows, {cases.opt(ctx.options)}"
            shape, dtype = (ctx.batch, ins[0].shape[-1]), self.held[0].dtype
            self.call = lambda out, stream: plan.apply_ptr(self.held[0].data_ptr(), self.held[1].data_ptr(), self.held[2].data_ptr(), out.data_ptr(), rows, stream)
        ctx_batch = ctx.batch
        self.replayed = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        self.eager = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            self.call(self.eager, side.cuda_stream)
        side.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.call(self.replayed, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    def after(self, i, ctx, case, ins, y):
        if i == history.CAPTURE_AT:
            self.y = y  # what the sequence's own call gave for these inputs, and what the fresh handle was compared with
            self.plan, self.options = ctx.plan, dict(ctx.options)

    def replay(self):
        """the graph and the eager call side by side, on the handle as the sequence left it but for the route options of the captured
        call; the delay handle first gets other delays and weights in the buffers the graph points at"""
        torch = self.torch
        if self.rule.handle == "delay":
            for key, value in self.options.items():
                self.plan.set_option(key, value)
            for held in self.held[1:]:
                held.copy_(torch.flip(held, (0,)) * 0.75 + 0.125)
        self.eager.fill_(float("nan"))
        torch.cuda.synchronize()
        self.graph.replay()
        self.call(self.eager, 0)
        torch.cuda.synchronize()
        return self.replayed.cpu().numpy(), self.eager.cpu().numpy()


@pytest.mark.parametrize("name", history.CAPTURABLE)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_a_graph_captured_after_half_the_sequence_replays_after_the_rest(torch, api, real, name):
    rule = history.GROUP[name][0]
    hooks = Captures(torch, api, rule)
    history.check_history(api, name, real, hooks)
    assert hooks.graph is not None
    replayed, eager = hooks.replay()
    bad = cases.differing(replayed, eager), cases.differing(replayed, hooks.y.reshape(replayed.shape))
    print(f"history {real} {name}: captured before call {history.CAPTURE_AT} ({hooks.what}), replayed after call "
          f"{history.CALLS - 1}: {bad[0]} reals differ from the eager call, {bad[1]} from call {history.CAPTURE_AT} itself")
    assert bad[0] == 0
    # the core call replays on the same input: the bits of call CAPTURE_AT; the delay call on OTHER delays and weights: not those
    assert (bad[1] == 0) == (rule.handle == "core"), bad


# ---- in place at a grid of four times the resident workgroups
class BigDeviceApi(DeviceApi):
    """DeviceApi whose run() can start from an output that holds `fill` (schedule_cases.InPlace) instead of NaN"""

    def run(self, call, shape, dtype, fill=None):
        count = int(np.prod(shape))
        buf = self.torch.full((count + 2 * cases.GUARD,), cases.SENTINEL, dtype=self.torch.from_numpy(np.empty(0, dtype)).dtype, device="cuda")
        out = buf[cases.GUARD:cases.GUARD + count]
        if fill is None:
            out.fill_(float("nan"))
        else:
            out.copy_(fill.reshape(-1))
        self.torch.cuda.synchronize()
        call(out.data_ptr())  # on the null stream
        self.torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.all(host[:cases.GUARD] == cases.SENTINEL) and np.all(host[-cases.GUARD:] == cases.SENTINEL), "a guard element was written"
        return host[cases.GUARD:cases.GUARD + count].reshape(shape).copy()


ARRAY_BYTES = 64 << 20     # the least a call's input (and output) takes
ALLOWANCE = 448 << 20      # the most: a test array stays below 512 MiB
PER_CU = 8                 # the workgroups of 256 threads a compute unit can hold at most: 32 waves of 4 waves each
TARGET = 4 * 256 * PER_CU  # four times what 256 compute units hold
IN_PLACE_NAMES = [c.name for c in cases.CASES if schedule.in_place(c)]


def workgroups_per_row(d, values):
    """A LOWER estimate of the workgroups one row (item) of `values` values gives the smallest grid of a call described as d.  No entry
    point reports a grid, so this is stated from what the kernels are, per route as describe() names it:
      tile passes   "AxB[xC] f32" not followed by "one-launch": a pass of length L over the M / L columns of a row takes a workgroup
                    per 16 columns at most (f64: 8) -- counted for the LONGEST pass, which has the fewest columns: M / (16 Lmax)
      everything else (one-launch, register stages, LDS mixed-radix, whole rows, and the sweeps around them, a workgroup per 256
                    values): one workgroup a row, and values / 256 where a row is shorter than that (the lane-per-transform and
                    small-row kernels pack 16 and more rows into a workgroup)"""
    least = min(1.0, values / 256.0)
    tiled = [[int(v) for v in m.group(1).split("x")] for m in re.finditer(r"(\d+(?:x\d+)+) f(?:32|64)", d)]
    if tiled:
        least = min(max(1, int(np.prod(t)) // (16 * max(t))) for t in tiled)
    return least


@pytest.mark.parametrize("name", IN_PLACE_NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_in_place_equals_out_of_place_at_a_grid_of_four_times_the_resident_workgroups(torch, real, name):
    """Every in-place call include/fourier.h allows (schedule_cases.IN_PLACE), on every route, at a batch sized so that the smallest
    grid of the call is at least TARGET = 4 x 256 compute units x PER_CU workgroups by workgroups_per_row's lower estimate -- at least
    ARRAY_BYTES, and at most ALLOWANCE an array, where the line printed says how far the estimate gets (f64 rows of 4096 and more
    points: 3.5 x): bit-equal to the out-of-place call of the same handle on the same rows (the table's rows, repeated).

    This asserts NOTHING about the order of execution -- on the device the order is the hardware's and a hazard shows by timing only.
    It only widens the window: the table's batch of 3 is a handful of workgroups, all resident together; here most of every grid
    waits for workgroups in front of it to retire.  PER_CU is the bound for workgroups of four waves; the kernels with one-wave
    workgroups serve rows of up to 64 points, whose batches here are sixteen times TARGET."""
    import fourier_amd

    api = BigDeviceApi(torch, fourier_amd)
    case = cases.BY_NAME[name]
    ctx = case.make(api, real)
    small = cases.rounded(case.unit_inputs(ctx), real)
    rows = small[0].shape[0]
    routes = case.routes(real)
    per_row = min(workgroups_per_row(case.select(ctx, real, options, prefix), small[0][0].size) for options, prefix in routes)
    need = int(np.ceil(TARGET / per_row))  # rows
    times = int(min(max(-(-need // rows), ARRAY_BYTES // small[0].nbytes), ALLOWANCE // small[0].nbytes))
    ins = [np.ascontiguousarray(np.tile(a, (times,) + (1,) * (a.ndim - 1))) if a.shape[0] == rows else a for a in small]
    ctx.batch = cases.BATCH * times
    reach = ins[0].shape[0] * per_row / (256 * PER_CU)
    assert ins[0].nbytes <= ALLOWANCE and ins[0].shape[0] == rows * times
    assert reach >= 4 or (times + 1) * small[0].nbytes > ALLOWANCE, (reach, "short of four times with room left")
    worst = 0
    for options, prefix in routes:
        d = case.select(ctx, real, options, prefix)
        y0 = case.run(api, ctx, ins)
        y = schedule.run_in_place(api, case, ctx, ins)
        bad = cases.differing(y, y0)
        worst = max(worst, bad)
        print(f"history {real} {name} {cases.opt(options)}in place at {ins[0].shape[0]} rows ({ins[0].nbytes >> 20} MiB), at least {per_row:g} workgroups a row: "
              f"{reach:.1f} x the resident {256 * PER_CU}; {bad} reals differ from out of place  [{d.split(':')[0]}]")
    assert worst == 0
