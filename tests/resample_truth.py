"""f64 numpy truth of the resampling tests (tests/test_resample_emu.py, tests/test_gpu_resample.py): the definition of include/fourier.h by
np.fft in f64 on the rounded input.  No torch FFT, no GPU.  N = x.shape[-1], M = num, K = min(N, M), W an optional window of N reals in
FFT order.

    complex rows: X = fft(x) * W;  Y[f mod M] = X[f mod N] for 2 |f| < K;  even K, h = K / 2:  M < N: Y[h] = X[h] + X[N-h],
                  N < M: Y[h] = Y[M-h] = X[h] / 2,  N == M: Y[h] = X[h];  y = ifft(Y) * M / N
    real rows:    X = rfft(x) * Wr, Wr[0] = W[0], Wr[k] = (W[k] + W[N-k]) / 2;  Y[k] = X[k] for 2 k < K;  even K: Y[K/2] = X[K/2] * c,
                  c = 2 (M < N), 1/2 (N < M), 1 (N == M);  y = irfft(Y, M) * M / N

which is scipy.signal.resample(x, M, axis=-1, window=W) apart from complex rows with M == 2 < N (scipy 1.15 leaves X[N-1] out of Y[1]
there; tests/test_resample_emu.py cross-checks this file against scipy and leaves exactly those cases out)."""
import numpy as np


def rows(rng, batch, n, dtype, complex_rows=False):
    """seeded white Gaussian rows, rounded to `dtype` (a real dtype; complex rows get both parts)"""
    x = rng.standard_normal((batch, n)).astype(dtype)
    if complex_rows:
        x = x + 1j * rng.standard_normal((batch, n)).astype(dtype)
    return np.ascontiguousarray(x)


def window(rng, n, dtype):
    """seeded window of uniform values in [0.5, 1.5], rounded to `dtype`"""
    return np.ascontiguousarray(rng.uniform(0.5, 1.5, n).astype(dtype))


def resample(x, m, w=None):
    """x: (batch, N) reals or complex values -> (batch, M) float64 / complex128"""
    x = np.asarray(x)
    n = x.shape[-1]
    k = min(n, m)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (n,)
    if np.iscomplexobj(x):
        X = np.fft.fft(x.astype(np.complex128), axis=-1) * w
        Y = np.zeros(x.shape[:-1] + (m,), np.complex128)
        for f in range(-(k // 2), k // 2 + 1):
            if 2 * abs(f) < k:
                Y[..., f % m] = X[..., f % n]
        if k % 2 == 0:
            h = k // 2
            if m < n:
                Y[..., h] = X[..., h] + X[..., n - h]
            elif n < m:
                Y[..., h] = X[..., h] / 2
                Y[..., m - h] = X[..., h] / 2
            else:
                Y[..., h] = X[..., h]
        return np.fft.ifft(Y, axis=-1) * (m / n)
    wr = np.empty(n // 2 + 1)
    wr[0] = w[0]
    for j in range(1, n // 2 + 1):
        wr[j] = (w[j] + w[n - j]) / 2
    X = np.fft.rfft(x.astype(np.float64), axis=-1) * wr
    Y = np.zeros(x.shape[:-1] + (m // 2 + 1,), np.complex128)
    for j in range(m // 2 + 1):
        if 2 * j < k:
            Y[..., j] = X[..., j]
    if k % 2 == 0:
        Y[..., k // 2] = X[..., k // 2] * (2.0 if m < n else 0.5 if n < m else 1.0)
    return np.fft.irfft(Y, m, axis=-1) * (m / n)
