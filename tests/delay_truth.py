"""f64 numpy truth of the delay tests (tests/test_delay_emu.py, tests/test_gpu_delay.py): the definition of include/fourier.h by
np.fft.fft / ifft in f64 on the inputs, delays and weights AS ROUNDED to the handle's type.  No torch FFT, no GPU.

    X = fft(x, L),  Y[g] = sum_c w[gC + c] X[gC + c] m(., d[gC + c]),  out[g] = ifft(Y[g])[:n]
    m(k, d) = exp(-2 pi i k' d / L),  k' = k for k < L/2, k - L for k > L/2;  m(L/2, d) = cos(pi d)  (even L)

The phase is formed from d mod L (fmod of the f64 value is exact), so that the truth itself loses nothing at huge delays.
Checked (test_truth_* of tests/test_delay_emu.py): integer d with L >= n + d reproduces the shifted row to 1e-14, L == n reproduces
numpy.roll, and a bin-centred cosine delayed by 0.3 samples comes out to 3e-14."""
import numpy as np

DELAYS = (0.0, 1.0, -2.5, 0.37, 1234.625, -7.001)  # the delays of every batch of 6 rows


def rows(rng, batch, n, dtype):
    """seeded white Gaussian rows, rounded to `dtype` (real or complex)"""
    v = rng.standard_normal((batch, n))
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal((batch, n))
    return np.ascontiguousarray(v.astype(dtype))


def multiplier(L, d):
    """m(k, d) for every bin k and every delay of the 1-D array d: shape (len(d), L), complex128"""
    d = np.fmod(np.asarray(d, dtype=np.float64), float(L))  # exact
    k = np.arange(L)
    kp = np.where(2 * k < L, k, k - L).astype(np.float64)
    di = np.rint(d)
    df = d - di  # exact
    # whole turns of k' d_int drop out: the integer exponent is exact in int64, the fraction is at most a quarter turn
    e = np.mod(np.outer(di.astype(np.int64), k), L).astype(np.float64)
    m = np.exp(-2j * np.pi * (e + np.outer(df, kp)) / L)
    if L % 2 == 0:
        m[:, L // 2] = np.where(np.mod(di, 2) == 0, 1.0, -1.0) * np.cos(np.pi * df)  # cos(pi d) = (-1)^d_int cos(pi d_frac)
    return m


def delay(x, d, L, channels=1, weights=None):
    """the handle's output in f64 / complex128: x of shape (batch, n), one delay (and weight) per row -> (batch / channels, n)"""
    x = np.asarray(x)
    real = np.dtype(x.dtype).kind != "c"
    batch, n = x.shape
    assert batch % channels == 0 and L >= n
    X = np.fft.fft(x.astype(np.float64 if real else np.complex128), L, axis=-1)
    w = np.ones(batch) if weights is None else np.asarray(weights, dtype=np.float64)
    Y = (w[:, None] * X * multiplier(L, d)).reshape(batch // channels, channels, L).sum(axis=1)
    y = np.fft.ifft(Y, axis=-1)[:, :n]
    return np.ascontiguousarray(y.real if real else y)


def norms(x, channels=1, weights=None):
    """sum_c |w_c| ||x_c||_2 per output row: the denominator of the measure"""
    x = np.asarray(x)
    batch = x.shape[0]
    w = np.ones(batch) if weights is None else np.abs(np.asarray(weights, dtype=np.float64))
    nrm = np.linalg.norm(x.astype(np.complex128), axis=-1)
    return (w * nrm).reshape(batch // channels, channels).sum(axis=1)


def err(got, want, x, channels=1, weights=None):
    """max over output rows of ||got - want||_2 / sum_c |w_c| ||x_c||_2: rigorous for any n <= L, since every |m| <= 1"""
    diff = np.linalg.norm(np.asarray(got).astype(np.complex128) - want, axis=-1)
    return float(np.max(diff / norms(x, channels, weights)))
