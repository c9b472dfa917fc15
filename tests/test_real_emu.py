"""Real-input transforms (fourier_hip_real_*, fourier_amd.RealFft) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against numpy's rfft / irfft.
The `-m gpu` twin is tests/test_gpu_real.py."""
import ctypes

import numpy as np
import pytest

from helpers import rel_l2

CODES_FWD = (0, 3)      # FFT, SQRT_SCALED_FFT
CODES_INV = (1, 2, 4)   # IFFT, UNSCALED_IFFT, SQRT_SCALED_IFFT
INVALID = 1             # FOURIER_HIP_INVALID_ARGUMENT
SIZES = list(range(1, 65)) + [96, 100, 255, 256, 486, 1000, 1001, 4096]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def want_forward(x, code):
    y = np.fft.rfft(x.astype(np.float64), axis=-1)
    return y / np.sqrt(x.shape[-1]) if code == 3 else y


def want_inverse(X, n, code):
    y = np.fft.irfft(X.astype(np.complex128), n=n, axis=-1)
    return {1: y, 2: n * y, 4: np.sqrt(n) * y}[code]


def forward(plan, x, code=0):
    x = np.ascontiguousarray(x)
    out = np.empty(x.shape[:-1] + (plan.size() // 2 + 1,), np.complex128 if x.dtype == np.float64 else np.complex64)
    plan.forward_batch_ptr(x.ctypes.data, out.ctypes.data, x.shape[0], code)
    return out


def inverse(plan, X, code=1):
    X = np.ascontiguousarray(X)
    out = np.empty(X.shape[:-1] + (plan.size(),), np.float64 if X.dtype == np.complex128 else np.float32)
    plan.inverse_batch_ptr(X.ctypes.data, out.ctypes.data, X.shape[0], code)
    return out


def hermitian_input(rng, batch, n):
    return np.fft.rfft(rng.standard_normal((batch, n)), axis=-1)


@pytest.mark.parametrize("sizes", [SIZES[i::4] for i in range(4)], ids=["a", "b", "c", "d"])
def test_forward_and_inverse_match_numpy_for_every_code(fa, sizes):
    rng = np.random.default_rng(7)
    for n in sizes:
        plan = fa.create_rfft_f64(n)
        x = rng.standard_normal((3, n))
        for code in CODES_FWD:
            got = forward(plan, x, code)
            assert rel_l2(got, want_forward(x, code)) <= 1e-12, (n, code)
        X = hermitian_input(rng, 3, n)  # a real signal's spectrum
        X[:, 1:] += 0.25 * (rng.standard_normal((3, n // 2)) + 1j * rng.standard_normal((3, n // 2)))  # ... and any half spectrum
        for code in CODES_INV:
            got = inverse(plan, X, code)
            assert rel_l2(got, want_inverse(X, n, code)) <= 1e-12, (n, code)


def test_f32_plans_match_numpy(fa):
    rng = np.random.default_rng(8)
    for n in (1, 2, 7, 16, 30, 64, 100, 1001, 4096):
        plan = fa.create_rfft_f32(n)
        x = rng.standard_normal((3, n)).astype(np.float32)
        assert rel_l2(forward(plan, x, 0), want_forward(x, 0)) <= 4e-6, n
        X = hermitian_input(rng, 3, n).astype(np.complex64)
        assert rel_l2(inverse(plan, X, 1), want_inverse(X, n, 1)) <= 4e-6, n


def test_round_trip_returns_the_input(fa):
    rng = np.random.default_rng(9)
    for n in (1, 2, 3, 8, 33, 64, 486, 1001, 4096):
        plan = fa.create_rfft_f64(n)
        x = rng.standard_normal((3, n))
        assert np.allclose(inverse(plan, forward(plan, x, 0), 1), x, rtol=0, atol=1e-12), n
        assert np.allclose(inverse(plan, forward(plan, x, 3), 4), x, rtol=0, atol=1e-12), n


def test_imaginary_parts_of_dc_and_nyquist_are_ignored(fa):
    rng = np.random.default_rng(10)
    for n in (1, 2, 5, 8, 9, 64, 255, 256):
        plan = fa.create_rfft_f64(n)
        X = hermitian_input(rng, 3, n)
        noisy = X.copy()
        noisy[:, 0] += 1j * rng.standard_normal(3)
        if n % 2 == 0:
            noisy[:, n // 2] += 1j * rng.standard_normal(3)
        for code in CODES_INV:
            assert np.allclose(inverse(plan, noisy, code), inverse(plan, X, code), rtol=0, atol=1e-12), (n, code)


def test_inverse_leaves_its_input_unchanged(fa):
    rng = np.random.default_rng(11)
    for n in (6, 7, 64, 1000, 1001):
        plan = fa.create_rfft_f64(n)
        X = hermitian_input(rng, 3, n)
        X[:, 0] += 1j
        before = X.tobytes()
        inverse(plan, X, 1)
        assert X.tobytes() == before, n


def test_describe_names_the_path_and_the_inner_plan(fa):
    for n in (2, 64, 100, 4096):
        assert fa.create_rfft_f64(n).describe() == "real half-length: " + fa.create_fft_f64(n // 2).describe()
        assert fa.create_rfft_f32(n).describe() == "real half-length: " + fa.create_fft_f32(n // 2).describe()
    for n in (1, 15, 1001):
        assert fa.create_rfft_f64(n).describe() == "real full-length: " + fa.create_fft_f64(n).describe()


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    assert not L.fourier_hip_real_create_float(0, -1) and not L.fourier_hip_real_create_double(0, -1)
    with pytest.raises(fa.FourierError):
        fa.create_rfft_f32(0)
    assert L.fourier_hip_real_size_double(None) == 0
    assert L.fourier_hip_real_describe_double(None) == b""
    assert L.fourier_hip_real_last_status_double(None) == INVALID
    assert L.fourier_hip_real_forward_batch_double(None, 16, 16, 1, 0, None) == INVALID
    assert L.fourier_hip_real_reserve_double(None, 1) == INVALID
    L.fourier_hip_real_destroy_double(None)

    n = 16
    plan = fa.create_rfft_f64(n)
    h = plan._h
    x = np.zeros((2, n))
    X = np.zeros((2, n // 2 + 1), np.complex128)
    big = np.zeros(4 * n + 8)
    fwd, inv = L.fourier_hip_real_forward_batch_double, L.fourier_hip_real_inverse_batch_double
    for code in CODES_INV:
        assert fwd(h, x.ctypes.data, X.ctypes.data, 2, code, None) == INVALID
    for code in CODES_FWD + (5, -1):
        assert inv(h, X.ctypes.data, x.ctypes.data, 2, code, None) == INVALID
    assert L.fourier_hip_real_last_status_double(h) == INVALID
    assert fwd(h, x.ctypes.data, X.ctypes.data, 2, 0, None) == 0
    assert L.fourier_hip_real_last_status_double(h) == 0  # reset on entry
    assert fwd(h, big.ctypes.data, big.ctypes.data, 1, 0, None) == INVALID              # in place
    assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * 16, 2, 0, None) == INVALID     # partial overlap
    assert fwd(h, big.ctypes.data + 8, X.ctypes.data, 1, 0, None) == INVALID            # 8-byte aligned, 16 needed
    assert inv(h, X.ctypes.data, big.ctypes.data + 8, 1, 1, None) == INVALID
    assert fwd(h, None, X.ctypes.data, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data, None, 1, 1, None) == INVALID
    assert fwd(h, x.ctypes.data, X.ctypes.data, 0, 0, None) == 0                        # batch 0: no-op
    with pytest.raises(fa.FourierError):
        plan.forward_batch_ptr(x.ctypes.data, X.ctypes.data, 2, fa.Transform.Ifft)
    f32 = fa.create_rfft_f32(n)
    xf = np.zeros(2 * n + 2, np.float32)
    Xf = np.zeros(n, np.complex64)
    assert L.fourier_hip_real_forward_batch_float(f32._h, xf.ctypes.data + 4, Xf.ctypes.data, 1, 0, None) == INVALID
    assert L.fourier_hip_real_forward_batch_float(f32._h, xf.ctypes.data + 8, Xf.ctypes.data, 1, 0, None) == 0


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(12)
    for n in (8, 64, 255, 1000, 1001, 4096):
        plan = fa.create_rfft_f64(n)
        plan.reserve(5)
        x = rng.standard_normal((5, n))
        X = hermitian_input(rng, 5, n)
        before = L.fourier_emu_alloc_count()
        for b in (1, 5, 3):
            for code in CODES_FWD:
                forward(plan, x[:b], code)
            for code in CODES_INV:
                inverse(plan, X[:b], code)
        assert L.fourier_emu_alloc_count() == before, n


def test_batches_larger_than_one_scratch_chunk(fa, monkeypatch):
    rng = np.random.default_rng(13)
    for n in (16, 15, 2, 1):
        per = (n // 2 if n % 2 == 0 else n) * 16 or 16
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(2 * per))  # two rows per chunk: a batch of 7 in four chunks
        plan = fa.create_rfft_f64(n)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        x = rng.standard_normal((7, n))
        for code in CODES_FWD:
            assert rel_l2(forward(plan, x, code), want_forward(x, code)) <= 1e-12, (n, code)
        X = hermitian_input(rng, 7, n)
        for code in CODES_INV:
            assert rel_l2(inverse(plan, X, code), want_inverse(X, n, code)) <= 1e-12, (n, code)
