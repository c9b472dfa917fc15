"""No result depends on the order of execution, WITHOUT a GPU: tests/schedule_cases.py on the CPU emulation (tests/emu), whose
launches take a schedule (tests/emu/hipemu.h: Schedule) -- the thread order between two barriers, the block order, and shuffles that
wait for their own wave only.  Every (case, precision, route) of tests/amplitude_cases.py and every core plan kind, out of place and,
where the header allows it, in place, gives under each of the 14 other schedules the bits it gives under the default one, which are
held to the f64 truth once.  There is no GPU twin: on the device the order is the hardware's."""
import pytest

import amplitude_cases as cases
import schedule_cases as sched


@pytest.fixture(scope="module")
def api():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield sched.HostApi(fourier_amd)
    _lib._lib = prev


def test_the_counts_of_the_table():
    """the runs check 1 compares: the table's (case, precision, route) count times the number of schedules; nothing of it is exempt"""
    routes = sum(len(c.routes(real)) for c in cases.CASES for real in ("f32", "f64"))
    placed = sum(len(c.routes(real)) for c in cases.CASES for real in ("f32", "f64") if sched.in_place(c))
    total = sum(sched.table_runs(c, real) for c in cases.CASES for real in ("f32", "f64"))
    print(f"schedule table: {routes} (case, precision, route) x {len(sched.SCHEDULES)} schedules = {total} runs compared, 0 left out; "
          f"in place: {placed} x ({len(sched.SCHEDULES)} schedules + the default) = {placed * (len(sched.SCHEDULES) + 1)} more")
    assert total == routes * len(sched.SCHEDULES) and placed > 0
    assert {sched.family(c) for c in cases.CASES if sched.in_place(c)} == set(sched.IN_PLACE)  # every family of the list is met


def test_an_unknown_schedule_is_not_the_default(api):
    """a name the emulation does not know ends the process instead of running the default order under another name: tried in a child"""
    import subprocess
    import sys

    code = ("import sys; sys.path[:0] = %r; import numpy as np; from emu import build_emu; from fourier_amd import _lib; "
            "_lib._lib = build_emu.load(); import fourier_amd as fa; x = np.zeros((1, 64), np.complex64); "
            "fa.Fft(64, 'f32', -1).transform_batch_ptr(x.ctypes.data, x.copy().ctypes.data, 1, 0)" % sys.path)
    import os

    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HIPEMU_SCHEDULE="descendin:ascending"), capture_output=True, text=True)
    assert done.returncode != 0 and "names no schedule" in done.stderr, (done.returncode, done.stderr[-300:])


def test_every_exempt_name_is_a_route_of_the_build(api):
    """each word of WAITS_ON_OTHER_WORKGROUPS is shown by describe() of a plan this build can make, and has its reason"""
    seen = {sched.make_plan(api, k.n[real], real, k.env, k.options).describe() for k in sched.KINDS for real in ("f32", "f64")}
    for word, why in sched.WAITS_ON_OTHER_WORKGROUPS.items():
        assert why and any(word in d for d in seen), word


@pytest.mark.parametrize("name", cases.NAMES)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_the_table_under_every_schedule(api, real, name):
    sched.check_table(api, cases.BY_NAME[name], real)


@pytest.mark.parametrize("name", list(sched.KIND_BY_NAME))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_core_plan_kind_under_every_schedule(api, real, name):
    sched.check_kind(api, sched.KIND_BY_NAME[name], real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_register_stage_row_of_the_build_under_every_schedule(api, real):
    rows = sched.emu_register_rows(real)
    assert {bool(r.r3) for r in rows} == {False, True}, "two-stage and three-stage shapes"
    sched.check_rows(api, real, "register-stage rows", [(r.n, f"stockham registers {sched.kt.shape(r)} one-launch") for r in rows])


@pytest.mark.parametrize("part", range(sched.COVER_PARTS["plain"]))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_tile_pass_length_as_first_and_last_pass_under_two_schedules(api, real, part):
    """the rows of the plain cover table (tests/test_gpu_tables.py states what they cover): one transform each, COVER_SCHEDULES"""
    rows = sched.cover_rows("plain", real)[part::sched.COVER_PARTS["plain"]]
    assert rows
    sched.check_rows(api, real, f"tile cover 'plain' part {part}", rows, 1, sched.COVER_SCHEDULES)


@pytest.mark.parametrize("part", range(sched.COVER_PARTS["blu"]))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_tile_pass_length_in_the_bluestein_roles_under_two_schedules(api, real, part):
    """the rows of the Bluestein cover table: every tile-pass length as chirp-in / chirp-out pass and as conv pass, likewise"""
    rows = sched.cover_rows("blu", real)[part::sched.COVER_PARTS["blu"]]
    assert rows
    sched.check_rows(api, real, f"tile cover 'blu' part {part}", rows, 1, sched.COVER_SCHEDULES)


# ---- the schedules change the order that is executed: three toy launches (tests/emu/order_probe.cpp), one process per schedule
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import os
    import subprocess
    import sys

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
    exe = str(tmp_path_factory.mktemp("order_probe") / "order_probe")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-include", os.path.join(here, "hipemu.h"), os.path.join(here, "order_probe.cpp"), "-o", exe])

    def run(threads=None, blocks=None):
        env = {k: v for k, v in os.environ.items() if k != sched.ENV}
        env["HIPEMU_THREADS"] = "1"  # one worker: under the default too the blocks run one after the other, ascending
        if threads is not None:
            env[sched.ENV] = f"{threads}:{blocks}"
        done = subprocess.run([exe], env=env, capture_output=True, text=True, check=True)
        lines = dict(line.split(" ", 1) for line in done.stdout.strip().split("\n"))
        return {key: [float(v) for v in value.split()] for key, value in lines.items()}

    return run


def test_every_schedule_runs_the_threads_and_blocks_in_its_own_order(probe):
    """the log of (block, thread) visits of 3 blocks x 128 threads: the default is ascending in both; each thread order and each block
    order is a different order over the same visits, descending the exact reverse, waves-descending the waves reversed with their
    lanes ascending; if HIPEMU_SCHEDULE were not read, or every name meant the default, this fails"""
    ascending = [b * 1000 + t for b in range(3) for t in range(128)]
    assert probe()["visit"] == ascending == probe("ascending", "ascending")["visit"]
    seen = {}
    for threads in sched.THREADS:
        for blocks in sched.BLOCKS:
            visit = probe(threads, blocks)["visit"]
            assert sorted(visit) == ascending, (threads, blocks, "every thread of every block runs once")
            order_of_blocks = [int(v) // 1000 for v in visit[::128]]
            in_block = [int(v) % 1000 for v in visit[:128]]
            assert all([int(v) % 1000 for v in visit[k * 128:(k + 1) * 128]] == in_block for k in range(3))  # one thread order for every block
            seen[(threads, blocks)] = (tuple(order_of_blocks), tuple(in_block))
            if blocks == "ascending":
                assert order_of_blocks == [0, 1, 2]
            if blocks == "descending":
                assert order_of_blocks == [2, 1, 0]
            if threads == "descending":
                assert in_block == list(range(127, -1, -1))
            if threads == "waves-descending":
                assert in_block == list(range(64, 128)) + list(range(64))
    assert len({v[1] for v in seen.values()}) == len(sched.THREADS), "five different thread orders"
    assert len({v[0] for v in seen.values()}) == len(sched.BLOCKS), "three different block orders"
    print(f"schedule probe: {len(seen)} schedules, {len(set(seen.values()))} different orders of 384 visits")
    assert len(set(seen.values())) == len(seen) == 15


def test_a_sweep_that_reads_the_next_workgroups_row_fails_under_the_other_block_orders(probe):
    """an in-place sweep in which block b adds row b + 1 to row b (rows 1, 2, 4, 8, 16): right -- 3, 6, 12, 24, 16 -- where the blocks
    run in ascending order, under every thread order; wrong under every schedule whose block order is descending or permuted.  This
    is the fault the block orders exist for, and the default schedule cannot see it"""
    want = [3.0, 6.0, 12.0, 24.0, 16.0]
    assert probe()["sweep"] == want
    wrong = 0
    for threads, blocks in sched.SCHEDULES:
        got = probe(threads, blocks)["sweep"]
        assert (got == want) == (blocks == "ascending"), (threads, blocks, got)
        wrong += got != want
    print(f"schedule probe: the cross-workgroup sweep is right under the default and wrong under {wrong} of {len(sched.SCHEDULES)} schedules")
    assert wrong == 10


def test_a_missing_barrier_next_to_a_shuffle_fails_under_every_other_schedule(probe):
    """two waves exchange through LDS with a __shfl_xor but no __syncthreads() between the store and the load: the default schedule's
    shuffle is two whole-block barriers and hides it; under every other schedule a wave passes its shuffle alone, and the wave that
    runs first reads LDS the other has not written.  The shuffled value itself is right everywhere"""
    want, partner = [(t + 64) % 128 + 1 for t in range(128)], [t ^ 1 for t in range(128)]
    assert probe()["shuffle"] == want and probe()["partner"] == partner
    for threads, blocks in sched.SCHEDULES:
        got = probe(threads, blocks)
        assert got["shuffle"] != want, (threads, blocks, "the missing barrier stayed hidden")
        assert got["partner"] == partner, (threads, blocks, "the shuffle itself")
    print(f"schedule probe: the missing barrier next to a shuffle is hidden under the default and shows under all {len(sched.SCHEDULES)} schedules")
