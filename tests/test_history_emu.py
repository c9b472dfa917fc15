"""No result depends on the handle's call history, WITHOUT a GPU: tests/history_cases.py on the CPU emulation (tests/emu) -- the same
kernel sources in CPU arithmetic, driven through the same C ABI / Python layer as the product.  The `-m gpu` twin is
tests/test_gpu_history.py; the two run the same sequences and make the same assertion: every call of one handle that goes through
twelve calls of changing kind, route, batch, length and window gives, bit for bit, what a fresh handle gives for that call alone, and
the fresh handle's result is within the family's bound of the f64 truth."""
import pytest

import amplitude_cases as cases
import history_cases as history


@pytest.fixture(scope="module")
def api():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield cases.HostApi(fourier_amd)
    _lib._lib = prev


def test_every_case_is_in_exactly_one_group():
    seen = [c.name for rule, members in history.GROUP.values() for c in members]
    assert sorted(seen) == sorted(cases.NAMES)
    print(f"history groups: {len(history.GROUP)} handles serve the table's {len(seen)} cases")


@pytest.mark.parametrize("name", history.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_a_call_gives_what_a_fresh_handle_gives(api, real, name):
    history.check_history(api, name, real)


class CountsAllocations:
    """what the GPU twin's captured graph relies on: after history_cases.reserve_for_capture before call CAPTURE_AT, no later call of the handle allocates (a plan-owned buffer that moved would leave the graph pointing at freed
    memory)"""

    def __init__(self, lib, rule):
        self.lib, self.rule, self.at, self.later = lib, rule, None, 0

    def before_state(self, i, ctx):
        history.freeze_options(i, ctx)
        self.at = self.lib.fourier_emu_alloc_count()  # from here to after(): the history handle's setters, options and call

    def before(self, i, ctx, case, ins):
        if i == history.CAPTURE_AT:
            history.reserve_for_capture(ctx, self.rule)
            self.at = self.lib.fourier_emu_alloc_count()

    def after(self, i, ctx, case, ins, y):
        if i >= history.CAPTURE_AT:
            assert self.lib.fourier_emu_alloc_count() == self.at, (case.name, "call", i, "the handle allocated after the reserve")
            self.later += 1


@pytest.mark.parametrize("name", history.CAPTURABLE)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_no_call_allocates_after_the_reserve_the_graph_test_makes(api, real, name):
    from fourier_amd import _lib

    _lib._lib.fourier_emu_alloc_count.restype = __import__("ctypes").c_uint64
    hooks = CountsAllocations(_lib._lib, history.GROUP[name][0])
    history.check_history(api, name, real, hooks)
    assert hooks.later == history.CALLS - history.CAPTURE_AT
