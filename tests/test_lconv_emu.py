"""Linear convolution with a prepared filter bank (fourier_hip_lconv_*, fourier_amd.LinearConv) WITHOUT a GPU: the engine sources
compiled against the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against
numpy.convolve / numpy.correlate in f64 on the same (rounded) inputs, sliced to the mode.  The `-m gpu` twin is tests/test_gpu_lconv.py.

Tolerance, relative L2 over the whole output, three transforms' worth (the block's forward, the filter's forward, the inverse): 6e-6
(f32) and 3e-13 (f64) on the overlap-save route and on the padded route over an inner plan that is not a Bluestein one,
tests/test_conv_emu.py's (1.2e-5, 3e-12) over a Bluestein one.  The real pairing passes the same arithmetic as the complex kernel and has
no tolerance of its own."""
import ctypes

import numpy as np
import pytest

from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
TOL = {"f64": 3e-13, "f32": 6e-6}
TOL_BLUESTEIN = {"f64": 3 * 1e-12, "f32": 3 * 4e-6}  # tests/test_conv_emu.py's
MODES = ("full", "same", "valid")
SENTINEL = 77.0


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


def want(x, h, mode, correlate=False):
    """numpy in f64 on the rounded inputs, row b with filter b mod F, sliced by the table of include/fourier.h"""
    h = np.atleast_2d(h)
    lx, k = x.shape[-1], h.shape[-1]
    wide = np.complex128 if np.dtype(x.dtype).kind == "c" else np.float64
    off, lout = {"full": (0, lx + k - 1), "same": ((k - 1) // 2, lx), "valid": (k - 1, lx - k + 1)}[mode]
    rows = []
    for b in range(x.shape[0]):
        hb = h[b % h.shape[0]].astype(wide)
        if correlate:
            hb = np.conj(hb[::-1])
        rows.append(np.convolve(x[b].astype(wide), hb)[off:off + lout])
    return np.array(rows)


def tol(plan, real):
    return (TOL_BLUESTEIN if "bluestein" in plan.describe() else TOL)[real]


def run(plan, x, h, correlate=False):
    """set the filters and apply into a buffer with a guard row in front and behind; checks the guards and that nothing read was written"""
    h = np.ascontiguousarray(np.atleast_2d(h))
    bx, bh = x.tobytes(), h.tobytes()
    plan.set_filters_ptr(h.ctypes.data, h.shape[0], correlate)
    assert plan.filters() == h.shape[0]
    lout = plan.out_length()
    buf = np.full((x.shape[0] + 2, lout), SENTINEL, x.dtype)
    plan.apply_ptr(x.ctypes.data, buf[1:].ctypes.data, x.shape[0])
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx and h.tobytes() == bh, "apply modified its input or the taps"
    return buf[1:-1]


# (Lx, K): three blocks at 2^11 with a partial last one; odd rows and SAME offset 15; one block (real data: a pair with no second
# block); K > Lx (FULL only); K = 1; five blocks (an odd number >= 3 for the real pairing)
SHAPES = [(5000, 33), (4999, 32), (1900, 7), (40, 64), (3000, 1), (9000, 100)]


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_overlap_save_matches_numpy(fa, real, real_data):
    rng = np.random.default_rng(41)
    dt = dtype_of(real, real_data)
    for lx, k in SHAPES:
        for mode in MODES:
            if k > lx and mode != "full":
                continue
            plan = fa.LinearConv(lx, k, real, mode, real_data)
            assert plan.describe().startswith("lconv overlap-save: block 2048 "), plan.describe()
            x, h = rand(rng, (2, lx), dt), rand(rng, (1, k), dt)
            got = run(plan, x, h)
            w = want(x, h, mode)
            assert got.shape == w.shape
            assert rel_l2(got, w) <= tol(plan, real), (lx, k, mode, real_data, plan.describe())
    nb5 = fa.LinearConv(9000, 100, real, "full", real_data).describe()
    assert " blocks 5" in nb5 and ("real pairs" in nb5) == real_data, nb5


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
def test_forced_block_4096_with_1025_taps(fa, real_data):
    rng = np.random.default_rng(42)
    dt = dtype_of("f64", real_data)
    plan = fa.LinearConv(7000, 1025, "f64", "same", real_data)
    assert plan.describe().startswith("lconv overlap-save: block 4096 ")
    x, h = rand(rng, (3, 7000), dt), rand(rng, (2, 1025), dt)
    plan.set_option("block", 13)
    assert plan.describe().startswith("lconv overlap-save: block 8192 step 7168 blocks 2"), plan.describe()
    assert rel_l2(run(plan, x, h), want(x, h, "same")) <= tol(plan, "f64")
    plan.set_option("block", 12)
    assert plan.describe().startswith("lconv overlap-save: block 4096 step 3072 blocks 3"), plan.describe()
    with pytest.raises(fa.FourierError):
        plan.apply_ptr(x.ctypes.data, x.ctypes.data + x.nbytes, 1)  # the change of block dropped the bank
    assert rel_l2(run(plan, x, h), want(x, h, "same")) <= tol(plan, "f64")
    plan.set_option("block", 0)  # the rule picks the same block: the bank stays
    y = np.empty((3, 7000), dt)
    plan.apply_ptr(x.ctypes.data, y.ctypes.data, 3)
    assert rel_l2(y, want(x, h, "same")) <= tol(plan, "f64")


def test_route_choice(fa):
    def route(k, real, lx=70000):
        return fa.LinearConv(lx, k, real, "full").describe()

    for real in ("f32", "f64"):
        assert route(1, real).startswith("lconv overlap-save: block 2048 step 2048 ")
        assert route(257, real).startswith("lconv overlap-save: block 2048 ")
        assert route(4097, real).startswith("lconv overlap-save: block 16384 ")
    # f64: the smallest block of 4 (K - 1), to 2^14; then 2^14 while it holds 2 (K - 1)
    assert route(513, "f64").startswith("lconv overlap-save: block 2048 ")      # 4 (K - 1) = 2048
    assert route(514, "f64").startswith("lconv overlap-save: block 4096 ")
    assert route(1025, "f64").startswith("lconv overlap-save: block 4096 ")
    assert route(1026, "f64").startswith("lconv overlap-save: block 8192 ")
    assert route(4098, "f64").startswith("lconv overlap-save: block 16384 ")
    assert route(8193, "f64").startswith("lconv overlap-save: block 16384 ")
    assert route(8194, "f64").startswith("lconv padded: M=131072, conv ")
    # f32: first the smallest block of 8 (K - 1) up to 2^13, where the row is longer than that block ...
    assert route(258, "f32").startswith("lconv overlap-save: block 4096 ")      # 8 (K - 1) = 2056
    assert route(513, "f32").startswith("lconv overlap-save: block 4096 ")
    assert route(514, "f32").startswith("lconv overlap-save: block 8192 ")
    assert route(1025, "f32").startswith("lconv overlap-save: block 8192 ")     # 8 (K - 1) = 8192
    assert route(600, "f32", lx=4096).startswith("lconv overlap-save: block 4096 ")  # a row shorter than 8192: the 4 (K - 1) block
    # ... then the 4 (K - 1) steps, to 2^15; then 2^15 while it holds 2 (K - 1)
    assert route(1026, "f32").startswith("lconv overlap-save: block 8192 ")
    assert route(2049, "f32").startswith("lconv overlap-save: block 8192 ")
    assert route(2050, "f32").startswith("lconv overlap-save: block 16384 ")
    assert route(4098, "f32").startswith("lconv overlap-save: block 32768 ")
    assert route(8193, "f32").startswith("lconv overlap-save: block 32768 ")
    assert route(16385, "f32").startswith("lconv overlap-save: block 32768 ")    # 2 (K - 1) = 2^15
    assert route(16386, "f32").startswith("lconv padded: M=131072, conv ")
    # the step is a whole number of 128-byte lines of complex data
    assert " step 2032 " in route(17, "f32") and " step 2032 " in route(17, "f64")
    assert " step 2016 " in route(20, "f32") and " step 2024 " in route(20, "f64")


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
def test_padded_route(fa, real_data):
    rng = np.random.default_rng(43)
    for real in ("f32", "f64"):
        dt = dtype_of(real, real_data)
        for mode in MODES:
            plan = fa.LinearConv(300, 50, real, mode, real_data)
            plan.set_option("overlap_save", 0)
            assert plan.describe().startswith("lconv padded: M=512, conv "), plan.describe()
            x, h = rand(rng, (3, 300), dt), rand(rng, (2, 50), dt)
            for correlate in (False, True):
                assert rel_l2(run(plan, x, h, correlate), want(x, h, mode, correlate)) <= tol(plan, real), (real, mode, correlate)
            plan.set_option("overlap_save", 1)
            assert plan.describe().startswith("lconv overlap-save: ")
    for real in ("f32", "f64"):  # one value in, one tap: a circular handle of a single point
        dt = dtype_of(real, real_data)
        plan = fa.LinearConv(1, 1, real, "full", real_data)
        plan.set_option("overlap_save", 0)
        assert plan.describe().startswith("lconv padded: M=1, conv "), plan.describe()
        x, h = rand(rng, (5, 1), dt), rand(rng, (2, 1), dt)
        assert rel_l2(run(plan, x, h), want(x, h, "full")) <= tol(plan, real)
    dt = dtype_of("f32", real_data)
    plan = fa.LinearConv(30000, 20000, "f32", "full", real_data)
    assert plan.describe().startswith("lconv padded: M=65536, conv "), plan.describe()
    x, h = rand(rng, (2, 30000), dt), rand(rng, (1, 20000), dt)
    assert rel_l2(run(plan, x, h), want(x, h, "full")) <= tol(plan, "f32")


def test_padded_route_walks_chunks_with_the_right_filters(fa, monkeypatch):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(44)
    for real_data in (False, True):
        dt = dtype_of("f64", real_data)
        per = 512 * np.dtype(dt).itemsize
        monkeypatch.setenv("FOURIER_CONV_SCRATCH_BYTES", str(2 * per))  # two rows per chunk: a batch of 7 in four chunks
        plan = fa.LinearConv(300, 50, "f64", "same", real_data)
        monkeypatch.delenv("FOURIER_CONV_SCRATCH_BYTES")
        plan.set_option("overlap_save", 0)
        x, h = rand(rng, (7, 300), dt), rand(rng, (3, 50), dt)
        plan.set_filters_ptr(h.ctypes.data, 3)
        plan.reserve(2)  # buffers reserved for TWO rows serve a call of seven
        before = L.fourier_emu_alloc_count()
        y = np.empty((7, 300), dt)
        plan.apply_ptr(x.ctypes.data, y.ctypes.data, 7)
        assert L.fourier_emu_alloc_count() == before
        assert rel_l2(y, want(x, h, "same")) <= tol(plan, "f64")


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
def test_filter_bank_and_correlation(fa, real_data):
    rng = np.random.default_rng(45)
    dt = dtype_of("f64", real_data)
    for mode in MODES:
        plan = fa.LinearConv(2500, 33, "f64", mode, real_data)
        x, h = rand(rng, (7, 2500), dt), rand(rng, (3, 33), dt)
        for correlate in (False, True):
            w = want(x, h, mode, correlate)
            assert rel_l2(run(plan, x, h, correlate), w) <= tol(plan, "f64"), (mode, correlate)
            if correlate:  # numpy's own correlation, row 4 with filter 1
                assert rel_l2(w[4], np.correlate(x[4].astype(w.dtype), h[1].astype(w.dtype), mode)) <= 1e-14
    # replacing the bank takes effect
    h1 = rand(rng, (1, 33), dt)
    assert rel_l2(run(plan, x, h1), want(x, h1, "valid")) <= tol(plan, "f64")


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(46)
    for real_data, overlap_save in ((False, 1), (True, 1), (False, 0), (True, 0)):
        dt = dtype_of("f64", real_data)
        plan = fa.LinearConv(2100, 9, "f64", "full", real_data)
        plan.set_option("overlap_save", overlap_save)
        h = rand(rng, (2, 9), dt)
        plan.set_filters_ptr(h.ctypes.data, 2)
        plan.reserve(5)
        x = rand(rng, (5, 2100), dt)
        y = np.empty((5, plan.out_length()), dt)
        before = L.fourier_emu_alloc_count()
        for b in (1, 5, 2):
            plan.apply_ptr(x.ctypes.data, y.ctypes.data, b)
        assert L.fourier_emu_alloc_count() == before, (real_data, overlap_save)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    lx, k = 100, 5
    for real_data in (False, True):
        plan = fa.create_lconv_f64(lx, k, "full", real_data)
        h = plan._h
        dt = dtype_of("f64", real_data)
        val = np.dtype(dt).itemsize
        x = np.zeros((2, lx), dt)
        y = np.zeros((2, lx + k - 1), dt)
        taps = np.ones((2, k), dt)
        big = np.zeros(8 * (2 * lx + k), np.float64)
        setf, app, status = L.fourier_hip_lconv_set_filters_double, L.fourier_hip_lconv_apply_double, L.fourier_hip_lconv_last_status_double
        assert L.fourier_hip_lconv_length_double(h) == lx and L.fourier_hip_lconv_taps_double(h) == k
        assert L.fourier_hip_lconv_out_length_double(h) == lx + k - 1 and L.fourier_hip_lconv_filters_double(h) == 0
        assert app(h, x.ctypes.data, y.ctypes.data, 2, None) == INVALID              # no filters yet
        assert status(h) == INVALID
        assert setf(h, taps.ctypes.data, 0, 0, None) == INVALID                      # filters == 0
        assert setf(h, None, 2, 0, None) == INVALID
        assert setf(h, taps.ctypes.data + val // 2, 1, 0, None) == INVALID           # taps: one value of their kind
        assert L.fourier_hip_lconv_filters_double(h) == 0
        assert setf(h, taps.ctypes.data, 2, 0, None) == 0
        assert status(h) == 0 and L.fourier_hip_lconv_filters_double(h) == 2
        assert app(h, x.ctypes.data, y.ctypes.data, 2, None) == 0
        assert app(h, x.ctypes.data, x.ctypes.data, 2, None) == INVALID              # in place is not allowed
        assert status(h) == INVALID
        assert app(h, big.ctypes.data, big.ctypes.data + lx * val, 2, None) == INVALID      # the output begins inside the input
        assert app(h, big.ctypes.data + lx * val, big.ctypes.data, 2, None) == INVALID      # the input begins inside the output
        assert app(h, big.ctypes.data, big.ctypes.data + 2 * lx * val, 2, None) == 0        # adjacent, not overlapping
        assert status(h) == 0
        assert app(h, big.ctypes.data + val // 2, y.ctypes.data, 1, None) == INVALID        # misaligned
        assert app(h, x.ctypes.data, big.ctypes.data + val // 2, 1, None) == INVALID
        assert app(h, big.ctypes.data + val, y.ctypes.data, 1, None) == 0                   # one value of the kind is enough
        assert app(h, None, y.ctypes.data, 1, None) == INVALID
        assert app(h, x.ctypes.data, None, 1, None) == INVALID
        assert app(h, x.ctypes.data, y.ctypes.data, 0, None) == 0                    # batch 0: no-op
        opt = L.fourier_hip_lconv_set_option_double
        assert opt(h, b"block", 10) == INVALID and opt(h, b"block", 16) == INVALID
        assert opt(h, b"block", 15) == INVALID                                       # f64 has no 2^15 block
        assert opt(h, b"overlap_save", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
        assert plan.describe().startswith("lconv overlap-save: block 2048 ")         # a refused option leaves the handle as it was
        assert app(h, x.ctypes.data, y.ctypes.data, 2, None) == 0
        with pytest.raises(fa.FourierError):
            plan.apply_ptr(0, y.ctypes.data, 1)
    # a forced block must leave a step of at least one line
    p = fa.create_lconv_f32(70000, 2040, "full")
    assert L.fourier_hip_lconv_set_option_float(p._h, b"block", 11) == INVALID
    assert L.fourier_hip_lconv_set_option_float(p._h, b"block", 15) == 0
    p = fa.create_lconv_f32(70000, 2033, "full")
    assert L.fourier_hip_lconv_set_option_float(p._h, b"block", 11) == 0 and " step 16 " in p.describe()
