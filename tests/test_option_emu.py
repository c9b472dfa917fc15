"""The plan's options in combination and in any order, WITHOUT a GPU: tests/option_cases.py on the CPU emulation (tests/emu) -- the same
plan layer and kernel sources in CPU arithmetic, driven through the same C ABI / Python layer as the product.  The `-m gpu` twin is
tests/test_gpu_options.py; the two run the same tables and make the same assertions.  What only this twin can say: after a reserve no
call kind allocates under any combination of the two-pass options (the emulation counts allocations), and -- in a stand-alone program
under AddressSanitizer, tests/emu/option_probe.cpp -- no state of the two-pass matrix reads or writes outside a buffer."""
import ctypes
import os
import subprocess
import sys

import pytest

import option_cases as options
import schedule_cases as schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield schedule.HostApi(fourier_amd)
    _lib._lib = prev


@pytest.mark.parametrize("smooth_m", [0, 1, 2])
@pytest.mark.parametrize("name", options.BLU_NAMES)
def test_bluestein_options_in_any_order(api, oracle, name, smooth_m):
    options.check_bluestein(api, oracle, name, smooth_m)


@pytest.mark.parametrize("name", options.BLU_NAMES)
def test_bluestein_states_differ_where_the_rule_says_and_nowhere_else(api, name):
    options.check_bluestein_across_states(api, name)


@pytest.mark.parametrize("which", options.SEQUENCE_NAMES)
def test_a_sequence_gives_what_its_final_values_give(api, which):
    options.check_sequence(api, which)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_two_pass_options_in_combination(api, real):
    from fourier_amd import _lib

    _lib._lib.fourier_emu_alloc_count.restype = ctypes.c_uint64
    options.check_two_pass(api, real, alloc_count=_lib._lib.fourier_emu_alloc_count)


def test_a_profiled_call_of_a_pipelined_plan_with_scratch_has_its_scratch(api):
    """the state that wrote through a null scratch pointer: f32 2^16, "stream_pipeline" and "scratch" = 1, reserve(3), a profiled
    out-of-place call -- which does not pipeline and needs the scratch that prepare() did not size for a pipelined plan"""
    from fourier_amd import _lib

    _lib._lib.fourier_emu_alloc_count.restype = ctypes.c_uint64
    n = options.TWO_PASS["f32"][0]
    x = options.inputs(n, "f32", 3)
    plan = options.make(api, n, "f32", [("stream_pipeline", 2 | 2 << 16), ("scratch", 1)])
    plan.reserve(3)
    before = _lib._lib.fourier_emu_alloc_count()
    y, slots = options.call(api, plan, x, options.FFT, profiled=True)
    assert _lib._lib.fourier_emu_alloc_count() == before, "the profiled call allocated after the reserve"
    assert slots == ("pass0", "pass1"), slots
    assert options.cases.differing(y, options.call(api, options.make(api, n, "f32"), x, options.FFT)[0]) == 0


@pytest.mark.parametrize("which", list(options.OTHER_ROUTES))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_scratch_and_chunk_bytes_change_no_bit_on_every_other_route(api, monkeypatch, real, which):
    if which == "global passes":
        monkeypatch.setenv(*options.GLOBAL_PASS_ENV)
    options.check_other_route(api, which, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_register_stages_there_and_back_between_other_options(api, real):
    options.check_register_stages_interleaved(api, real)


def test_the_two_pass_matrix_in_a_stand_alone_program_under_the_address_sanitizer(api, tmp_path):
    """tests/emu/option_probe.cpp, linked with -fsanitize=address against the AddressSanitizer build of the emulation library (built
    by tests/emu/build_emu.py in a child process under FOURIER_EMU_ASAN=1), run as a child over every state of the two-pass matrix in
    both precisions -- the four call kinds, with and without the reserve -- and over the 48 Bluestein states at 10007 f64: exit status
    0, no report, and the bits of the in-process run.  (The sanitizer's options are those of tools/asan_emu.sh: the emulation's fibers
    switch stacks.)  The instrumented library and its objects are removed afterwards, as tools/asan_emu.sh removes them."""
    import shutil

    import numpy as np

    from emu import build_emu

    here = os.path.dirname(build_emu.__file__)
    leftovers = [os.path.join(here, name) for name in ("obj_asan", "libfourier_emu_asan.so", "libfourier_emu_asan.so.lock")]
    kept = [p for p in leftovers if os.path.exists(p)]  # somebody else's build in progress or in use stays
    try:
        prog = "import sys; sys.path[:0] = [%r, %r]; from emu import build_emu; print(build_emu.build())" % (os.path.join(ROOT, "tests"), ROOT)
        built = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, FOURIER_EMU_ASAN="1"), capture_output=True, text=True, timeout=3000)
        assert built.returncode == 0, built.stderr[-3000:]
        lib = built.stdout.strip().splitlines()[-1]
        assert lib.endswith("libfourier_emu_asan.so") and os.path.exists(lib), lib
        probe = str(tmp_path / "option_probe")
        linked = subprocess.run(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                                 os.path.join(here, "option_probe.cpp"), "-o", probe, lib, "-Wl,-rpath," + here, "-pthread"], capture_output=True, text=True, timeout=600)
        assert linked.returncode == 0, linked.stderr[-3000:]
        lines, expected = [], []
        for real in ("f32", "f64"):
            n = options.TWO_PASS[real][0]
            x = options.inputs(n, real, options.BATCH2)
            x.tofile(str(tmp_path / f"x_{real}"))
            base = options.call(api, options.make(api, n, real), x, options.FFT)[0]
            for index, state in enumerate(options.two_pass_states(real)):
                for kind in range(4):
                    out = str(tmp_path / f"y_{real}_{index}_{kind}")
                    lines.append(f"{n} {real} {options.BATCH2} {(index + kind) % 2} {kind} {options.FFT} {tmp_path / f'x_{real}'} {out} " +
                                 " ".join(f"{k}={v}" for k, v in zip(options.TWO_KEYS, state)))
                    expected.append((out, base, lines[-1]))
        blu = options.BLU_BY_NAME["10007 f64"]
        x = options.inputs(blu.n, blu.real, options.cases.BATCH)
        x.tofile(str(tmp_path / "x_blu"))
        for index, state in enumerate(options.BLU_STATES):
            settings = list(zip(options.BLU_KEYS, state))
            plan = options.make(api, blu.n, blu.real, settings)
            for kind, code in ((0, options.FFT), (3, options.IFFT)):
                out = str(tmp_path / f"y_blu_{index}_{kind}")
                lines.append(f"{blu.n} {blu.real} {options.cases.BATCH} {index % 2} {kind} {code} {tmp_path / 'x_blu'} {out} " + " ".join(f"{k}={v}" for k, v in settings))
                expected.append((out, options.call(api, plan, x, code)[0], lines[-1]))
        (tmp_path / "states").write_text("\n".join(lines) + "\n")
        # the caller's environment as it is, plus the sanitizer's options.  verify_asan_link_order=0: the runtime is linked into the probe
        # itself, so a library that the caller's environment preloads in front of it is no sign of a missing runtime
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:verify_asan_link_order=0")
        ran = subprocess.run([probe, str(tmp_path / "states")], env=env, capture_output=True, text=True, timeout=3000)
        assert ran.returncode == 0 and "AddressSanitizer" not in ran.stderr, (ran.returncode, ran.stdout[-500:], ran.stderr[-4000:])
        assert ran.stdout.strip() == f"option_probe: {len(lines)} states", ran.stdout
        bad = [line for out, want, line in expected if options.cases.differing(np.fromfile(out, want.dtype).reshape(want.shape), want)]
        print(f"options address-checked: {len(lines)} states in a stand-alone program, {len(bad)} differ from the in-process run")
        assert not bad, bad[:8]
    finally:
        for p in leftovers:
            if p not in kept:
                shutil.rmtree(p, ignore_errors=True) if os.path.isdir(p) else (os.path.exists(p) and os.remove(p))


def test_smooth13_of_0_and_1():
    """fourier_amd/warm_cache.py (as packaging/warm_cache.c): 0 is divisible by every prime, the loop over it never ended.  A host test
    with no library: the file is run by path in a child, so that a loop that does not end is a failure and not a hang of the suite."""
    prog = ("import importlib.util as u; s = u.spec_from_file_location('warm_cache', %r); m = u.module_from_spec(s); s.loader.exec_module(m); "
            "print([m.smooth13(v) for v in (0, 1, 2, 4459)])" % os.path.join(ROOT, "fourier_amd", "warm_cache.py"))
    out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "[False, False, True, True]", (out.stdout, out.stderr[-500:])
