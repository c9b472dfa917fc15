"""f64 numpy truth of the analytic-signal tests (tests/test_hilbert_emu.py, tests/test_gpu_hilbert.py): the definition of
include/fourier.h by np.fft.fft / ifft in f64 on the rounded input.  No torch FFT, no GPU.

    X = fft(x),  m[k] = 1 for k = 0 and (N even) k = N/2, 2 for 0 < k < N/2 (odd N: k <= (N-1)/2), 0 above,
    z = ifft(X * m),  envelope = |z|

which is scipy.signal.hilbert along the last axis (and not scipy.signal.envelope)."""
import numpy as np


def rows(rng, batch, n, dtype):
    """seeded white Gaussian rows, rounded to `dtype`"""
    return np.ascontiguousarray(rng.standard_normal((batch, n)).astype(dtype))


def multiplier(n):
    m = np.zeros(n)
    m[0] = 1.0
    if n % 2 == 0:
        m[n // 2] = 1.0
        m[1:n // 2] = 2.0
    else:
        m[1:(n + 1) // 2] = 2.0
    return m


def analytic(x):
    """x: (batch, N) reals -> (batch, N) complex128"""
    x = np.asarray(x, dtype=np.float64)
    return np.fft.ifft(np.fft.fft(x, axis=-1) * multiplier(x.shape[-1]), axis=-1)


def envelope(x):
    return np.abs(analytic(x))
