"""Real-input N-D transforms (fourier_hip_realnd_*, fourier_amd.RealFftN) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against numpy's rfftn / irfftn.
The `-m gpu` twin is tests/test_gpu_realnd.py."""
import ctypes

import numpy as np
import pytest

from helpers import rel_l2

CODES_FWD = (0, 3)      # FFT, SQRT_SCALED_FFT
CODES_INV = (1, 2, 4)   # IFFT, UNSCALED_IFFT, SQRT_SCALED_IFFT
INVALID, UNSUPPORTED = 1, 3  # FOURIER_HIP_INVALID_ARGUMENT, FOURIER_HIP_UNSUPPORTED

# leading lengths 1, 2, odd, even, prime and above 32 (lane, column-tile and transpose axis routes); even and odd W, W = 1, 2, 3
SHAPES = [
    (1, 8), (2, 8), (3, 6), (4, 2), (5, 1), (7, 3), (6, 4), (9, 5), (8, 64), (64, 128), (37, 10), (33, 12), (96, 16), (4, 1000),
    (3, 4, 6), (2, 5, 7), (5, 3, 2), (1, 4, 4), (4, 1, 10), (6, 64, 128), (3, 2, 3),
    (2, 3, 4, 6), (3, 2, 5, 5), (2, 2, 2, 2), (1, 3, 1, 8), (5, 4, 3, 9),
    (2,), (3,), (1,), (10,), (15,), (64,),
]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def axes_of(shape):
    return tuple(range(1, len(shape) + 1))


def want_forward(x, shape, code):
    y = np.fft.rfftn(x.astype(np.float64), axes=axes_of(shape))
    return y / np.sqrt(np.prod(shape)) if code == 3 else y


def want_inverse(X, shape, code):
    y = np.fft.irfftn(X.astype(np.complex128), s=shape, axes=axes_of(shape))
    p = float(np.prod(shape))
    return {1: y, 2: p * y, 4: np.sqrt(p) * y}[code]


def forward(plan, x, code=0):
    x = np.ascontiguousarray(x)
    out = np.full((x.shape[0],) + plan.half_shape(), np.nan, np.complex128 if x.dtype == np.float64 else np.complex64)
    plan.forward_batch_ptr(x.ctypes.data, out.ctypes.data, x.shape[0], code)
    return out


def inverse(plan, X, code=1):
    X = np.ascontiguousarray(X)
    out = np.full((X.shape[0],) + plan.shape, np.nan, np.float64 if X.dtype == np.complex128 else np.float32)
    plan.inverse_batch_ptr(X.ctypes.data, out.ctypes.data, X.shape[0], code)
    return out


def any_half_spectrum(rng, batch, shape, dtype=np.complex128):
    """Arbitrary complex values of the half-spectrum shape: not the spectrum of any real signal."""
    s = (batch,) + shape[:-1] + (shape[-1] // 2 + 1,)
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(dtype)


@pytest.mark.parametrize("shapes", [SHAPES[i::4] for i in range(4)], ids=["a", "b", "c", "d"])
def test_forward_and_inverse_match_numpy_for_every_code_f64(fa, shapes):
    rng = np.random.default_rng(21)
    for shape in shapes:
        plan = fa.RealFftN(shape, "f64")
        for batch in (1, 3):
            x = rng.standard_normal((batch,) + shape)
            for code in CODES_FWD:
                assert rel_l2(forward(plan, x, code), want_forward(x, shape, code)) <= 1e-12, (shape, batch, code)
            X = any_half_spectrum(rng, batch, shape)
            for code in CODES_INV:
                assert rel_l2(inverse(plan, X, code), want_inverse(X, shape, code)) <= 1e-12, (shape, batch, code)


@pytest.mark.parametrize("shapes", [SHAPES[i::2] for i in range(2)], ids=["a", "b"])
def test_forward_and_inverse_match_numpy_for_every_code_f32(fa, shapes):
    rng = np.random.default_rng(22)
    for shape in shapes:
        plan = fa.RealFftN(shape, "f32")
        x = rng.standard_normal((3,) + shape).astype(np.float32)
        for code in CODES_FWD:
            assert rel_l2(forward(plan, x, code), want_forward(x, shape, code)) <= 3e-6, (shape, code)
        X = any_half_spectrum(rng, 3, shape, np.complex64)
        for code in CODES_INV:
            assert rel_l2(inverse(plan, X, code), want_inverse(X, shape, code)) <= 3e-6, (shape, code)


def test_inverse_of_input_that_is_not_hermitian_matches_numpy(fa):
    """numpy's irfftn runs the leading inverses first and drops the imaginary parts of the last axis's bins 0 and W/2 afterwards:
    columns 0 and W/2 are projected over the leading axes.  The plain mirror formula (columns 0 and W/2 mixed) fails this."""
    rng = np.random.default_rng(23)
    for shape in ((4, 8), (5, 8), (6, 2), (3, 4, 6), (2, 3, 4, 4), (7, 7)):
        plan = fa.RealFftN(shape, "f64")
        X = any_half_spectrum(rng, 2, shape)
        want = np.fft.irfftn(X, s=shape, axes=axes_of(shape))
        assert rel_l2(inverse(plan, X), want) <= 1e-12, shape
        # the only parts of X that matter in columns 0 and W/2 are their Hermitian parts over the leading axes
        herm = np.fft.rfftn(want, axes=axes_of(shape))
        assert rel_l2(inverse(plan, herm), want) <= 1e-12, shape


def test_round_trip_returns_the_input(fa):
    rng = np.random.default_rng(24)
    for shape in ((4, 8), (3, 5), (2, 3, 6), (2, 2, 3, 4), (9,)):
        plan = fa.RealFftN(shape, "f64")
        x = rng.standard_normal((3,) + shape)
        assert np.allclose(inverse(plan, forward(plan, x, 0), 1), x, rtol=0, atol=1e-12), shape
        assert np.allclose(inverse(plan, forward(plan, x, 3), 4), x, rtol=0, atol=1e-12), shape


def test_rank_one_has_the_bits_of_the_real_plan(fa):
    rng = np.random.default_rng(25)
    for n in (1, 2, 3, 8, 15, 64, 100, 1001):
        for real, dt in (("f64", np.float64), ("f32", np.float32)):
            nd, one = fa.RealFftN((n,), real), fa.RealFft(n, real)
            assert nd.describe() == "realnd rank 1: " + one.describe()
            x = rng.standard_normal((3, n)).astype(dt)
            a, b = forward(nd, x), np.full((3, n // 2 + 1), np.nan, np.complex128 if real == "f64" else np.complex64)
            one.forward_batch_ptr(x.ctypes.data, b.ctypes.data, 3, 0)
            assert a.tobytes() == b.tobytes(), (n, real)
            X = a.copy()
            y, z = inverse(nd, X), np.full((3, n), np.nan, dt)
            one.inverse_batch_ptr(X.ctypes.data, z.ctypes.data, 3, 1)
            assert y.tobytes() == z.tobytes(), (n, real)


def test_inverse_leaves_its_input_unchanged(fa):
    rng = np.random.default_rng(26)
    for shape in ((4, 8), (3, 5), (2, 3, 6)):
        plan = fa.RealFftN(shape, "f64")
        X = any_half_spectrum(rng, 2, shape)
        before = X.tobytes()
        inverse(plan, X, 1)
        assert X.tobytes() == before, shape


def test_describe_names_the_route(fa):
    d = fa.RealFftN((64, 2048, 2048), "f32").describe()
    assert d.startswith("realnd packed: rows " + fa.create_fft_f32(1024).describe() + "; ")
    assert "axis 0 (64): axis column tile: L=64" in d and "axis 1 (2048): axis column tile: L=2048" in d
    d = fa.RealFftN((37, 10), "f64").describe()
    assert d == "realnd packed: rows " + fa.create_fft_f64(5).describe() + "; axis 0 (37): axis transpose: " + fa.create_fft_f64(37).describe()
    d = fa.RealFftN((16, 1, 10), "f64").describe()
    assert "axis 0 (16): axis lane: 16" in d and "axis 1 (1): identity" in d
    d = fa.RealFftN((4, 15), "f64").describe()
    assert d == "realnd composed: rows " + fa.create_rfft_f64(15).describe() + "; axis 0 (4): axis lane: 4"


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    shape = (ctypes.c_size_t * 5)(4, 4, 4, 4, 4)
    for create in (L.fourier_hip_realnd_create_float, L.fourier_hip_realnd_create_double):
        assert not create(0, shape, -1) and not create(5, shape, -1) and not create(-1, shape, -1)  # rank 0, 5, negative
        assert not create(2, None, -1)                                                              # NULL shape
        assert not create(2, (ctypes.c_size_t * 2)(4, 0), -1) and not create(2, (ctypes.c_size_t * 2)(0, 4), -1)  # size 0
        assert create(4, shape, -1)
    with pytest.raises(fa.FourierError):
        fa.RealFftN((2, 2, 2, 2, 2), "f64")
    with pytest.raises(fa.FourierError):
        fa.RealFftN((), "f64")
    assert L.fourier_hip_realnd_rank_double(None) == 0
    assert L.fourier_hip_realnd_describe_double(None) == b""
    assert L.fourier_hip_realnd_last_status_double(None) == INVALID
    assert L.fourier_hip_realnd_forward_batch_double(None, 16, 16, 1, 0, None) == INVALID
    assert L.fourier_hip_realnd_inverse_batch_double(None, 16, 16, 1, 1, None) == INVALID
    assert L.fourier_hip_realnd_reserve_double(None, 1) == INVALID
    L.fourier_hip_realnd_destroy_double(None)

    for shape in ((4, 16), (4, 15)):
        plan = fa.RealFftN(shape, "f64")
        assert L.fourier_hip_realnd_rank_double(plan._h) == 2 and plan.rank() == 2
        h = plan._h
        item, half = int(np.prod(shape)), shape[0] * (shape[1] // 2 + 1)
        x = np.zeros((2,) + shape)
        X = np.zeros((2,) + plan.half_shape(), np.complex128)
        big = np.zeros(4 * item + 8)
        fwd, inv = L.fourier_hip_realnd_forward_batch_double, L.fourier_hip_realnd_inverse_batch_double
        for code in CODES_INV + (5, -1):
            assert fwd(h, x.ctypes.data, X.ctypes.data, 2, code, None) == INVALID, code
        for code in CODES_FWD + (5, -1):
            assert inv(h, X.ctypes.data, x.ctypes.data, 2, code, None) == INVALID, code
        assert L.fourier_hip_realnd_last_status_double(h) == INVALID
        assert fwd(h, x.ctypes.data, X.ctypes.data, 2, 0, None) == 0
        assert L.fourier_hip_realnd_last_status_double(h) == 0  # reset on entry
        assert fwd(h, big.ctypes.data, big.ctypes.data, 1, 0, None) == INVALID                 # in place
        assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * item, 2, 0, None) == INVALID      # partial overlap
        assert inv(h, big.ctypes.data, big.ctypes.data + 16 * half - 16, 1, 1, None) == INVALID
        assert fwd(h, big.ctypes.data + 8, X.ctypes.data, 1, 0, None) == INVALID               # 8-byte aligned, 16 needed
        assert inv(h, X.ctypes.data, big.ctypes.data + 8, 1, 1, None) == INVALID
        assert fwd(h, None, X.ctypes.data, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data, None, 1, 1, None) == INVALID
        assert fwd(h, x.ctypes.data, X.ctypes.data, 0, 0, None) == 0                           # batch 0: no-op
        assert inv(h, X.ctypes.data, x.ctypes.data, 0, 1, None) == 0
        with pytest.raises(fa.FourierError):
            plan.forward_batch_ptr(x.ctypes.data, X.ctypes.data, 2, fa.Transform.Ifft)
        with pytest.raises(fa.FourierError):
            plan.inverse_batch_ptr(X.ctypes.data, x.ctypes.data, 2, fa.Transform.Fft)
    f32 = fa.RealFftN((2, 8), "f32")
    xf = np.zeros(40, np.float32)
    Xf = np.zeros(16, np.complex64)
    assert L.fourier_hip_realnd_forward_batch_float(f32._h, xf.ctypes.data + 4, Xf.ctypes.data, 1, 0, None) == INVALID
    assert L.fourier_hip_realnd_forward_batch_float(f32._h, xf.ctypes.data + 8, Xf.ctypes.data, 1, 0, None) == 0


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(27)
    for shape in ((8, 16), (37, 10), (4, 15), (3, 4, 6), (64, 128), (16,), (15,)):
        plan = fa.RealFftN(shape, "f64")
        plan.reserve(5)
        x = rng.standard_normal((5,) + shape)
        X = any_half_spectrum(rng, 5, shape)
        before = L.fourier_emu_alloc_count()
        for b in (1, 5, 3):
            for code in CODES_FWD:
                forward(plan, x[:b], code)
            for code in CODES_INV:
                inverse(plan, X[:b], code)
        assert L.fourier_emu_alloc_count() == before, shape


def test_batches_larger_than_one_scratch_chunk_and_items_larger_than_the_bound(fa, monkeypatch):
    rng = np.random.default_rng(28)
    for shape in ((4, 16), (3, 15), (2, 3, 8), (5, 2)):
        cols = shape[-1] // 2 if shape[-1] % 2 == 0 else shape[-1] // 2 + 1
        per = int(np.prod(shape[:-1])) * cols * 16
        for cap in (2 * per, per // 3):  # two items per chunk (a batch of 7 in four chunks); an item larger than the bound
            monkeypatch.setenv("FOURIER_REALND_SCRATCH_BYTES", str(cap))
            plan = fa.RealFftN(shape, "f64")
            monkeypatch.delenv("FOURIER_REALND_SCRATCH_BYTES")
            x = rng.standard_normal((7,) + shape)
            for code in CODES_FWD:
                assert rel_l2(forward(plan, x, code), want_forward(x, shape, code)) <= 1e-12, (shape, cap, code)
            X = any_half_spectrum(rng, 7, shape)
            for code in CODES_INV:
                assert rel_l2(inverse(plan, X, code), want_inverse(X, shape, code)) <= 1e-12, (shape, cap, code)


def test_dims_layout_helper():
    from fourier_amd.fft import realnd_layout

    assert realnd_layout(3, None) == ((0, 1, 2), None)
    assert realnd_layout(3, (-2, -1)) == ((1, 2), None)
    assert realnd_layout(4, (2, 1, 3)) == ((2, 1, 3), None)          # the trailing block in any order, the real axis last
    assert realnd_layout(3, (2,)) == ((2,), None)
    assert realnd_layout(3, (0, 1)) == ((0, 1), (2, 0, 1))           # batch dimension 2 to the front
    assert realnd_layout(3, (2, 1)) == ((2, 1), (0, 2, 1))           # the real axis not last
    assert realnd_layout(4, (3, 0, 2)) == ((3, 0, 2), (1, 0, 3, 2))
    assert realnd_layout(5, (-1, -2, -3, -4)) == ((4, 3, 2, 1), (0, 2, 3, 4, 1))
    for bad in ((), (3,), (-4,), (0, 0), (1, -2), (0, 1, 2, 3, 4)):
        with pytest.raises(ValueError):
            realnd_layout(5 if len(bad) == 5 else 3, bad)
