"""Transforms along a strided axis (fourier_hip_transform_axis_*, Fft.transform_axis_ptr) WITHOUT a GPU: the engine sources compiled
against the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against numpy's fft
along axis 1 of the [outer][N][inner] array.  The `-m gpu` twin is tests/test_gpu_axis.py."""
import ctypes
import os

import numpy as np
import pytest

from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
LANE = list(range(1, 33))
COLUMN = (64, 256, 1024)
TRANSPOSE = (33, 48, 97, 100, 243, 1000, 4096)


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def want(x, code):
    x = x.astype(np.complex128)
    n = x.shape[1]
    return {0: np.fft.fft(x, axis=1), 1: np.fft.ifft(x, axis=1), 2: n * np.fft.ifft(x, axis=1),
            3: np.fft.fft(x, axis=1) / np.sqrt(n), 4: np.sqrt(n) * np.fft.ifft(x, axis=1)}[code]


def signal(rng, outer, n, inner, dt):
    return (rng.standard_normal((outer, n, inner)) + 1j * rng.standard_normal((outer, n, inner))).astype(dt)


def run(plan, x, code, in_place=False):
    if in_place:
        y = x.copy()
        plan.transform_axis_ptr(y.ctypes.data, y.ctypes.data, x.shape[0], x.shape[2], code)
        return y
    y = np.empty_like(x)
    plan.transform_axis_ptr(x.ctypes.data, y.ctypes.data, x.shape[0], x.shape[2], code)
    return y


def expected_route(plan, n, inner, real):
    if inner == 1:
        return plan.describe()
    if n <= 32:
        return f"axis lane: {n}"
    cols = (32 if n <= 256 else 16) // (1 if real == "f32" else 2)  # the last pass's tile width (16-byte units of CG column groups)
    if n in (64, 128, 256, 512, 1024, 2048) and inner & (inner - 1) == 0 and inner >= cols:
        return f"axis column tile: L={n}"
    return "axis transpose: " + plan.describe()


def check_cases(fa, real, cases, tol, codes=range(5)):
    rng = np.random.default_rng(len(cases))
    dt = np.complex64 if real == "f32" else np.complex128
    create = fa.create_fft_f32 if real == "f32" else fa.create_fft_f64
    for n, inner, outer in cases:
        plan = create(n)
        assert plan.describe_axis(inner) == expected_route(plan, n, inner, real), (n, inner)
        x = signal(rng, outer, n, inner, dt)
        t = tol if (real == "f32" or "bluestein" not in plan.describe()) else 1e-11
        for code in codes:
            for in_place in (False, True):
                got = run(plan, x, code, in_place)
                assert rel_l2(got, want(x, code)) <= t, (n, inner, outer, real, code, in_place, plan.describe_axis(inner))


@pytest.mark.parametrize("part", range(4))
def test_lane_route_matches_numpy_f64(fa, part):
    inners = (2, 7, 16, 17, 48)
    cases = [(n, inners[i % len(inners)], 1 + 2 * (i % 2)) for i, n in enumerate(LANE) if i % 4 == part]
    check_cases(fa, "f64", cases, 1e-12)


def test_column_tile_route_matches_numpy_f64(fa):
    check_cases(fa, "f64", [(n, inner, outer) for n in COLUMN for inner, outer in ((16, 3), (64, 1))], 1e-12)


@pytest.mark.parametrize("part", range(2))
def test_transpose_route_matches_numpy_f64(fa, part):
    inners = (2, 7, 16, 17, 48)
    cases = [(n, inners[i % len(inners)], 1 + 2 * (i % 2)) for i, n in enumerate(TRANSPOSE)]
    # power-of-two lengths with a ragged inner, and inner 1 (the plan's own route)
    cases += [(64, 7, 3), (256, 17, 1), (1024, 48, 1), (100, 1, 3), (64, 1, 2)]
    check_cases(fa, "f64", cases[part::2], 1e-12)


def test_f32_cases_match_numpy(fa):
    cases = [(1, 7, 3), (3, 16, 1), (16, 48, 1), (31, 17, 3), (32, 2, 3), (64, 16, 3), (2048, 16, 1), (1000, 7, 1), (97, 48, 1),
             (128, 17, 3), (48, 1, 3)]
    check_cases(fa, "f32", cases, 4e-6, codes=(0, 1, 3))


def test_inner_one_is_the_batched_transform_bit_for_bit(fa):
    rng = np.random.default_rng(3)
    for real, n in (("f64", 64), ("f64", 1000), ("f32", 4096), ("f32", 97), ("f64", 7)):
        plan = (fa.create_fft_f32 if real == "f32" else fa.create_fft_f64)(n)
        x = signal(rng, 3, n, 1, np.complex64 if real == "f32" else np.complex128)
        for code in range(5):
            ref = np.empty_like(x)
            plan.transform_batch_ptr(x.ctypes.data, ref.ctypes.data, 3, code)
            assert run(plan, x, code).tobytes() == ref.tobytes(), (real, n, code)
        assert plan.describe_axis(1) == plan.describe()


def test_forced_transpose_route_agrees_with_the_automatic_one(fa, monkeypatch):
    rng = np.random.default_rng(4)
    for real, n, inner in (("f64", 5, 16), ("f64", 32, 7), ("f64", 17, 2), ("f64", 256, 16), ("f32", 64, 32), ("f32", 12, 48)):
        create = fa.create_fft_f32 if real == "f32" else fa.create_fft_f64
        auto = create(n)
        monkeypatch.setenv("FOURIER_AXIS_ROUTE", "transpose")
        forced = create(n)
        monkeypatch.delenv("FOURIER_AXIS_ROUTE")
        assert not auto.describe_axis(inner).startswith("axis transpose")
        assert forced.describe_axis(inner) == "axis transpose: " + forced.describe()
        x = signal(rng, 3, n, inner, np.complex64 if real == "f32" else np.complex128)
        tol = 4e-6 if real == "f32" else 1e-12
        for code in range(5):
            a, b = run(auto, x, code), run(forced, x, code)
            assert rel_l2(a, b) <= tol, (real, n, inner, code)
            assert rel_l2(b, want(x, code)) <= tol, (real, n, inner, code)


def test_calls_after_reserve_axis_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(5)
    for n, inner in ((7, 16), (64, 16), (100, 7), (4096, 2), (64, 7), (100, 1)):
        plan = fa.create_fft_f64(n)
        plan.reserve_axis(3, inner)
        x = signal(rng, 3, n, inner, np.complex128)
        before = L.fourier_emu_alloc_count()
        for outer in (1, 3, 2):
            for code in range(5):
                run(plan, x[:outer], code)
                run(plan, x[:outer], code, in_place=True)
        assert L.fourier_emu_alloc_count() == before, (n, inner, plan.describe_axis(inner))


def test_scratch_bound_forces_chunks_by_block_and_by_column_range(fa, monkeypatch):
    rng = np.random.default_rng(6)
    for n, inner, cap in ((100, 7, 2 * 100 * 7 * 16),   # two outer blocks per chunk: 5 blocks in three chunks
                          (100, 7, 3 * 100 * 16),       # one block in column ranges of three columns
                          (48, 17, 48 * 16),            # ... of one column
                          (4096, 3, 2 * 4096 * 16)):    # ... of two columns, the last range ragged
        monkeypatch.setenv("FOURIER_AXIS_SCRATCH_BYTES", str(cap))
        plan = fa.create_fft_f64(n)
        monkeypatch.delenv("FOURIER_AXIS_SCRATCH_BYTES")
        x = signal(rng, 5, n, inner, np.complex128)
        for code in range(5):
            for in_place in (False, True):
                assert rel_l2(run(plan, x, code, in_place), want(x, code)) <= 1e-12, (n, inner, cap, code, in_place)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    assert L.fourier_hip_transform_axis_double(None, 16, 16, 1, 2, 0, None) == INVALID
    assert L.fourier_hip_reserve_axis_double(None, 1, 2) == INVALID
    assert L.fourier_hip_describe_axis_double(None, 2) == b""
    n, inner = 16, 4
    plan = fa.create_fft_f64(n)
    h = plan._h
    x = np.zeros((2, n, inner), np.complex128)
    y = np.zeros_like(x)
    big = np.zeros(4 * n * inner + 2, np.complex128)
    f = L.fourier_hip_transform_axis_double
    for code in (5, -1):
        assert f(h, x.ctypes.data, y.ctypes.data, 2, inner, code, None) == INVALID
    assert L.fourier_hip_last_status_double(h) == INVALID
    assert f(h, x.ctypes.data, y.ctypes.data, 2, inner, 0, None) == 0
    assert L.fourier_hip_last_status_double(h) == 0  # reset on entry
    assert f(h, big.ctypes.data, big.ctypes.data + 16 * n, 2, inner, 0, None) == INVALID    # partial overlap
    assert L.fourier_hip_last_status_double(h) == INVALID
    assert f(h, big.ctypes.data, big.ctypes.data, 2, inner, 0, None) == 0                   # in place
    assert f(h, big.ctypes.data + 8, y.ctypes.data, 1, inner, 0, None) == INVALID           # 8-byte aligned, 16 needed
    assert f(h, x.ctypes.data, big.ctypes.data + 8, 1, inner, 0, None) == INVALID
    assert f(h, None, y.ctypes.data, 1, inner, 0, None) == INVALID
    assert f(h, x.ctypes.data, None, 1, inner, 0, None) == INVALID
    before = y.copy()
    assert f(h, x.ctypes.data, y.ctypes.data, 0, inner, 0, None) == 0                       # outer 0: no-op
    assert f(h, x.ctypes.data, y.ctypes.data, 2, 0, 0, None) == 0                           # inner 0: no-op
    assert y.tobytes() == before.tobytes()
    with pytest.raises(fa.FourierError):
        plan.transform_axis_ptr(x.ctypes.data, y.ctypes.data, 2, inner, 7)
    f32 = fa.create_fft_f32(n)
    xf = np.zeros(2 * n * inner + 2, np.complex64)
    assert L.fourier_hip_transform_axis_float(f32._h, xf.ctypes.data + 4, xf.ctypes.data + 4, 1, inner, 0, None) == INVALID
    assert L.fourier_hip_transform_axis_float(f32._h, xf.ctypes.data + 8, xf.ctypes.data + 8, 1, inner, 0, None) == 0


def test_transpose_kernel_lds_is_bank_conflict_free(fa):
    """Bank-conflict model of MI355X_MICROARCH.md (the emulator's LDS trace) on transpose-route calls whose inner plan is itself
    exactly conflict-free there (tests/test_engine_emu.py: row-mode lengths 64, 128, 512): the transpose kernel is what is measured."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, ctypes; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from emu import build_emu\n"
        "from fourier_amd import _lib\n"
        "c = build_emu.load(); _lib._lib = c\n"
        "import fourier_amd as fa\n"
        "a, b, d = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()\n"
        "for n, real, outer, inner in ((64, 'f32', 2, 37), (128, 'f32', 1, 48), (512, 'f32', 1, 17), (128, 'f64', 2, 17), (512, 'f64', 1, 7)):\n"
        "    p = (fa.create_fft_f32 if real == 'f32' else fa.create_fft_f64)(n)\n"
        "    assert p.describe_axis(inner).startswith('axis transpose'), p.describe_axis(inner)\n"
        "    x = np.ones((outer, n, inner), np.complex64 if real == 'f32' else np.complex128); y = np.empty_like(x)\n"
        "    c.fourier_emu_lds_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(d), 1)\n"
        "    p.transform_axis_ptr(x.ctypes.data, y.ctypes.data, outer, inner, 0)\n"
        "    c.fourier_emu_lds_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(d), 1)\n"
        "    print(n, real, b.value / d.value)\n"
    ) % (os.path.dirname(here), here)
    env = dict(os.environ, HIPEMU_LDS_TRACE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.strip().splitlines() if len(l.split()) == 3]
    assert len(rows) == 5, out.stdout
    for n, real, ratio in rows:
        assert float(ratio) <= 1.05, (n, real, ratio)
