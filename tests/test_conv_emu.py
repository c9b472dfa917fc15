"""Convolution with a prepared filter bank (fourier_hip_conv_*, fourier_amd.FftConv) WITHOUT a GPU: the engine sources compiled
against the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against numpy in f64
on the same (rounded) inputs.  The `-m gpu` twin is tests/test_gpu_conv.py.

Tolerance, relative L2 over the whole output: three times the single-transform tolerance of tests/test_real_emu.py (1e-12 in f64,
4e-6 in f32), because three transforms in T contribute (the row's forward, the filter's forward, the inverse)."""
import ctypes

import numpy as np
import pytest

from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
TOL = {"f64": 3 * 1e-12, "f32": 3 * 4e-6}
SIZES = list(range(1, 65)) + [96, 100, 255, 256, 486, 1000, 1001, 2048, 4096, 16384]
SIZES_F32 = [1, 2, 3, 7, 16, 30, 64, 100, 255, 1000, 1001, 2048, 16384]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def dtype_of(real, real_data):
    if real_data:
        return np.float64 if real == "f64" else np.float32
    return np.complex128 if real == "f64" else np.complex64


def rand(rng, shape, dt):
    x = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return np.ascontiguousarray(x.astype(dt))


def want(x, h, correlate):
    """numpy in f64 on the rounded inputs; row b with filter b mod F"""
    n = x.shape[-1]
    h = np.atleast_2d(h)
    hb = h[np.arange(x.shape[0]) % h.shape[0]]
    if np.dtype(x.dtype).kind == "c":
        H = np.fft.fft(hb.astype(np.complex128), n, axis=-1)
        return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * (np.conj(H) if correlate else H), axis=-1)
    H = np.fft.rfft(hb.astype(np.float64), n, axis=-1)
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * (np.conj(H) if correlate else H), n=n, axis=-1)


def set_filters(plan, h, correlate=False):
    h = np.ascontiguousarray(np.atleast_2d(h))
    plan.set_filters_ptr(h.ctypes.data, h.shape[1], h.shape[0], correlate)


def apply(plan, x, in_place=False):
    if in_place:
        y = x.copy()
        plan.apply_ptr(y.ctypes.data, y.ctypes.data, y.shape[0])
        return y
    y = np.empty_like(x)
    plan.apply_ptr(x.ctypes.data, y.ctypes.data, x.shape[0])
    return y


def sweep_sizes(fa, real, sizes, seed):
    rng = np.random.default_rng(seed)
    for n in sizes:
        for real_data in (False, True):
            dt = dtype_of(real, real_data)
            plan = fa.FftConv(n, real, real_data)
            x = rand(rng, (7, n), dt)
            cases = [(taps, F, correlate) for taps in sorted({1, min(3, n), n}) for F in (1, 3) for correlate in (False, True)]
            for taps, F, correlate in cases:
                h = rand(rng, (F, taps), dt)
                set_filters(plan, h, correlate)
                assert plan.filters() == F
                w = want(x, h, correlate)
                for in_place in (False, True):
                    got = apply(plan, x, in_place)
                    assert rel_l2(got, w) <= TOL[real], (n, real_data, taps, F, correlate, in_place, plan.describe())


@pytest.mark.parametrize("sizes", [SIZES[i::4] for i in range(4)], ids=["a", "b", "c", "d"])
def test_f64_matches_numpy_for_every_length(fa, sizes):
    sweep_sizes(fa, "f64", sizes, 21)


def test_f32_matches_numpy(fa):
    sweep_sizes(fa, "f32", SIZES_F32, 22)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_two_pass_power_of_two_runs_the_fused_passes(fa, real):
    n = 1 << 16
    rng = np.random.default_rng(23)
    dt = dtype_of(real, False)
    plan = fa.FftConv(n, real)
    assert plan.describe() == "conv fused passes: " + fa.Fft(n, real).describe()
    x = rand(rng, (2, n), dt)
    h = rand(rng, (2, 129), dt)
    set_filters(plan, h, True)
    w = want(x, h, True)
    fused = apply(plan, x)
    assert rel_l2(fused, w) <= TOL[real]
    assert rel_l2(apply(plan, x, in_place=True), w) <= TOL[real]
    plan.set_option("fusion", 0)
    assert plan.describe() == "conv composed: " + fa.Fft(n, real).describe()
    composed = apply(plan, x)
    assert rel_l2(composed, w) <= TOL[real]
    assert rel_l2(fused, composed) <= TOL[real]


def test_a_two_pass_plan_that_is_not_a_palindrome_runs_the_fused_passes(fa):
    n = 1 << 15  # f64: 256 x 128, the inverse runs the mirrored plan
    rng = np.random.default_rng(24)
    plan = fa.FftConv(n, "f64")
    assert plan.describe() == "conv fused passes: " + fa.Fft(n, "f64").describe()
    x = rand(rng, (3, n), np.complex128)
    h = rand(rng, (2, 7), np.complex128)
    set_filters(plan, h)
    assert rel_l2(apply(plan, x), want(x, h, False)) <= TOL["f64"]


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_route_is_named_and_agrees_with_its_composed_form(fa, real):
    rng = np.random.default_rng(25)
    # (n, real data, the route "fusion" = 1 takes, the route "fusion" = 0 takes)
    for n, real_data, fused, composed in ((1000, False, "conv composed: ", "conv composed: "),
                                          (1024, False, "conv composed: ", "conv composed: "),
                                          (2048, False, "conv one-launch: ", "conv composed: "),
                                          (4096, False, "conv one-launch: ", "conv composed: "),
                                          (16384, False, "conv one-launch: ", "conv composed: "),
                                          (1000, True, "conv real fused untangle: ", "conv real composed: "),
                                          (4096, True, "conv real fused untangle: ", "conv real composed: "),
                                          (1001, True, "conv real composed: ", "conv real composed: ")):
        dt = dtype_of(real, real_data)
        plan = fa.FftConv(n, real, real_data)
        inner = fa.Fft(n // 2, real).describe() if real_data and n % 2 == 0 else None
        if fused == "conv real fused untangle: ":
            assert plan.describe() == fused + inner
        elif real_data:
            assert plan.describe() == fused + fa.RealFft(n, real).describe()
        else:
            assert plan.describe() == fused + fa.Fft(n, real).describe()
        x = rand(rng, (5, n), dt)
        h = rand(rng, (3, 17), dt)
        set_filters(plan, h)
        w = want(x, h, False)
        a = apply(plan, x)
        plan.set_option("fusion", 0)
        assert plan.describe().startswith(composed)
        if real_data:
            assert plan.describe() == composed + fa.RealFft(n, real).describe()
        b = apply(plan, x)
        plan.set_option("fusion", 1)
        assert plan.describe().startswith(fused)
        assert rel_l2(a, w) <= TOL[real] and rel_l2(b, w) <= TOL[real] and rel_l2(a, b) <= TOL[real], (n, real_data)
        with pytest.raises(fa.FourierError):
            plan.set_option("fusion", 2)
        with pytest.raises(fa.FourierError):
            plan.set_option("no_such_option", 1)


def test_filter_selection_across_chunk_boundaries(fa, monkeypatch):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(26)
    for n, real_data in ((16, False), (15, False), (16, True), (15, True), (2, True), (1, True), (1, False)):
        per = ((n // 2 + 1) if real_data else n) * 16
        monkeypatch.setenv("FOURIER_CONV_SCRATCH_BYTES", str(2 * per))  # two rows per chunk: a batch of 7 in four chunks
        plan = fa.FftConv(n, "f64", real_data)
        monkeypatch.delenv("FOURIER_CONV_SCRATCH_BYTES")
        dt = dtype_of("f64", real_data)
        x = rand(rng, (7, n), dt)
        h = rand(rng, (3, min(3, n)), dt)
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            set_filters(plan, h)
            # the bound was read and the batch is walked in chunks: buffers reserved for TWO rows serve a call of seven
            plan.reserve(2)
            before = L.fourier_emu_alloc_count()
            for in_place in (False, True):
                assert rel_l2(apply(plan, x, in_place), want(x, h, False)) <= TOL["f64"], (n, real_data, fusion, in_place)
            assert L.fourier_emu_alloc_count() == before, (n, real_data, fusion)


def test_fused_passes_walk_chunks_with_the_right_filters(fa, monkeypatch):
    n = 1 << 16
    rng = np.random.default_rng(27)
    monkeypatch.setenv("FOURIER_CONV_SCRATCH_BYTES", str(2 * 2 * n * 16))  # two rows per chunk on the fused-passes route
    plan = fa.FftConv(n, "f64")
    monkeypatch.delenv("FOURIER_CONV_SCRATCH_BYTES")
    assert plan.describe().startswith("conv fused passes: ")
    x = rand(rng, (5, n), np.complex128)
    h = rand(rng, (3, 4), np.complex128)
    set_filters(plan, h)
    assert rel_l2(apply(plan, x), want(x, h, False)) <= TOL["f64"]


def test_replacing_the_bank_takes_effect_and_inputs_stay_unchanged(fa):
    rng = np.random.default_rng(28)
    for n, real_data in ((64, False), (100, True), (33, True), (1000, False)):
        dt = dtype_of("f64", real_data)
        plan = fa.FftConv(n, "f64", real_data)
        x = rand(rng, (7, n), dt)
        before_x = x.tobytes()
        for F, taps, correlate in ((1, 5, False), (3, n, False), (2, 1, True), (1, 5, True)):
            h = rand(rng, (F, taps), dt)
            before_h = h.tobytes()
            set_filters(plan, h, correlate)
            assert plan.filters() == F
            assert rel_l2(apply(plan, x), want(x, h, correlate)) <= TOL["f64"], (n, real_data, F, taps, correlate)
            assert h.tobytes() == before_h and x.tobytes() == before_x


def test_an_impulse_returns_the_input_and_a_shifted_impulse_rotates_it(fa):
    rng = np.random.default_rng(29)
    for n, real_data in ((64, False), (100, True), (37, True), (1 << 16, False)):
        dt = dtype_of("f64", real_data)
        plan = fa.FftConv(n, "f64", real_data)
        x = rand(rng, (2, n), dt)
        set_filters(plan, np.ones((1, 1), dt))
        assert rel_l2(apply(plan, x), x) <= TOL["f64"]
        h = np.zeros((1, 3), dt)
        h[0, 2] = 1
        set_filters(plan, h)
        assert rel_l2(apply(plan, x), np.roll(x, 2, axis=-1)) <= TOL["f64"]
        set_filters(plan, h, correlate=True)
        assert rel_l2(apply(plan, x), np.roll(x, -2, axis=-1)) <= TOL["f64"]


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(30)
    for n, real_data in ((8, False), (64, True), (255, True), (1000, False), (1001, True), (4096, True), (1 << 16, False)):
        dt = dtype_of("f64", real_data)
        plan = fa.FftConv(n, "f64", real_data)
        batch = 5 if n < 65536 else 2
        set_filters(plan, rand(rng, (2, 3), dt))
        plan.reserve(batch)
        x = rand(rng, (batch, n), dt)
        before = L.fourier_emu_alloc_count()
        for b in (1, batch, 2):
            apply(plan, x[:b])
            apply(plan, x[:b], in_place=True)
        assert L.fourier_emu_alloc_count() == before, (n, real_data)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    for real_data in (0, 1):
        assert not L.fourier_hip_conv_create_float(0, real_data, -1) and not L.fourier_hip_conv_create_double(0, real_data, -1)
    with pytest.raises(fa.FourierError):
        fa.create_conv_f32(0)
    assert L.fourier_hip_conv_size_double(None) == 0
    assert L.fourier_hip_conv_filters_double(None) == 0
    assert L.fourier_hip_conv_describe_double(None) == b""
    assert L.fourier_hip_conv_last_status_double(None) == INVALID
    assert L.fourier_hip_conv_apply_double(None, 16, 16, 1, None) == INVALID
    assert L.fourier_hip_conv_set_filters_double(None, 16, 1, 1, 0, None) == INVALID
    assert L.fourier_hip_conv_reserve_double(None, 1) == INVALID
    assert L.fourier_hip_conv_set_option_double(None, b"fusion", 1) == INVALID
    L.fourier_hip_conv_destroy_double(None)

    n = 16
    for real_data in (False, True):
        plan = fa.create_conv_f64(n, real_data)
        h = plan._h
        dt = dtype_of("f64", real_data)
        row = n * np.dtype(dt).itemsize
        x = np.zeros((2, n), dt)
        y = np.zeros((2, n), dt)
        taps = np.ones((2, 3), dt)
        big = np.zeros(8 * n + 8, np.float64)
        setf, app, status = L.fourier_hip_conv_set_filters_double, L.fourier_hip_conv_apply_double, L.fourier_hip_conv_last_status_double
        assert L.fourier_hip_conv_size_double(h) == n and L.fourier_hip_conv_filters_double(h) == 0
        assert app(h, x.ctypes.data, y.ctypes.data, 2, None) == INVALID          # no filters yet
        assert status(h) == INVALID
        assert L.fourier_hip_conv_filters_double(h) == 0 and status(h) == INVALID  # a pure query leaves the status alone
        assert setf(h, taps.ctypes.data, 0, 2, 0, None) == INVALID               # taps == 0
        assert setf(h, taps.ctypes.data, n + 1, 1, 0, None) == INVALID           # taps > N
        assert setf(h, taps.ctypes.data, 3, 0, 0, None) == INVALID               # filters == 0
        assert setf(h, None, 3, 2, 0, None) == INVALID
        # taps are aligned to one value of their kind (complex 16 bytes, real 8 in f64): conv_pad_kernel reads them with plain loads
        assert setf(h, taps.ctypes.data + (4 if real_data else 8), 1, 1, 0, None) == INVALID
        assert status(h) == INVALID and L.fourier_hip_conv_filters_double(h) == 0
        assert setf(h, taps.ctypes.data, 3, 2, 0, None) == 0
        assert status(h) == 0 and L.fourier_hip_conv_filters_double(h) == 2     # reset on entry
        assert app(h, x.ctypes.data, y.ctypes.data, 2, None) == 0
        assert app(h, x.ctypes.data, x.ctypes.data, 2, None) == 0                # in place
        assert app(h, big.ctypes.data, big.ctypes.data + row // 2 // 16 * 16 + 16, 2, None) == INVALID  # partial overlap
        assert status(h) == INVALID
        assert app(h, big.ctypes.data, big.ctypes.data + 2 * row, 2, None) == 0  # adjacent, not overlapping
        assert status(h) == 0
        assert app(h, big.ctypes.data + 8, y.ctypes.data, 1, None) == INVALID    # 8-byte aligned, 16 needed (also for real rows)
        assert app(h, x.ctypes.data, big.ctypes.data + 8, 1, None) == INVALID
        assert app(h, None, y.ctypes.data, 1, None) == INVALID
        assert app(h, x.ctypes.data, None, 1, None) == INVALID
        assert app(h, x.ctypes.data, y.ctypes.data, 0, None) == 0                # batch 0: no-op
        assert L.fourier_hip_conv_set_option_double(h, b"fusion", 7) == INVALID
        assert L.fourier_hip_conv_set_option_double(h, None, 1) == INVALID
        with pytest.raises(fa.FourierError):
            plan.apply_ptr(0, y.ctypes.data, 1)
    f32 = fa.create_conv_f32(n, True)
    xf = np.zeros(2 * n + 2, np.float32)
    yf = np.zeros(n, np.float32)
    tf = np.ones(3, np.float32)
    assert L.fourier_hip_conv_set_filters_float(f32._h, tf.ctypes.data, 3, 1, 0, None) == 0
    assert L.fourier_hip_conv_apply_float(f32._h, xf.ctypes.data + 4, yf.ctypes.data, 1, None) == INVALID
    assert L.fourier_hip_conv_apply_float(f32._h, xf.ctypes.data + 8, yf.ctypes.data, 1, None) == 0
