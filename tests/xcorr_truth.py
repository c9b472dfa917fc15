"""f64 numpy truth of the cross-correlation tests (tests/test_xcorr_emu.py, tests/test_gpu_xcorr.py): the definition of
include/fourier.h by np.fft.fft / ifft in f64 on the rounded inputs.  No torch FFT, no GPU.

    X = fft(x, L),  Y = fft(y, L),  G = conj(X) Y,
    r = ifft(G)                                    (no weighting)
    r = ifft(conj(X / |X|) (Y / |Y|)), a bin 0 where |X| or |Y| is 0   (PHAT)
    out[j] = r[(lag_first + j) mod L],  j < lags

L >= 2n - 1, lag_first = -(n - 1), lags = 2n - 1 is numpy.correlate(y, x, "full")."""
import numpy as np


def rows(rng, batch, n, dtype):
    """seeded white Gaussian rows, rounded to `dtype` (real or complex)"""
    v = rng.standard_normal((batch, n))
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal((batch, n))
    return np.ascontiguousarray(v.astype(dtype))


def spike_rows(rng, batch, n, d, dtype):
    """x = a unit impulse at n // 3 plus noise of sigma 0.1 / sqrt(n); y = x delayed by d samples (zero fill) plus independent noise of
    the same sigma: the rows of the PHAT tests, whose spectra have no small bins"""
    sigma = 0.1 / np.sqrt(n)
    x = sigma * rng.standard_normal((batch, n))
    x[:, n // 3] += 1.0
    y = np.zeros_like(x)
    if d >= 0:
        y[:, d:] = x[:, :n - d]
    else:
        y[:, :n + d] = x[:, -d:]
    y += sigma * rng.standard_normal((batch, n))
    return np.ascontiguousarray(x.astype(dtype)), np.ascontiguousarray(y.astype(dtype))


def full(x, y, L, phat=False):
    """all L lags r[l] in f64 / complex128; real rows give a real array"""
    real = np.dtype(np.asarray(x).dtype).kind != "c"
    wide = np.float64 if real else np.complex128
    X = np.fft.fft(np.asarray(x, dtype=wide), L, axis=-1)
    Y = np.fft.fft(np.asarray(y, dtype=wide), L, axis=-1)
    if phat:
        ax, ay = np.abs(X), np.abs(Y)
        ok = ~((ax == 0) | (ay == 0))  # a NaN magnitude is not 0: the bin stays NaN (tests/isolation_cases.py)
        G = np.where(ok, np.conj(X / np.where(ok, ax, 1.0)) * (Y / np.where(ok, ay, 1.0)), 0.0)
    else:
        G = np.conj(X) * Y
    r = np.fft.ifft(G, axis=-1)
    return r.real if real else r


def window(r, lag_first, lags):
    L = r.shape[-1]
    return r[..., (lag_first + np.arange(lags)) % L]


def correlate(x, y, L, lag_first, lags, phat=False):
    return window(full(x, y, L, phat), lag_first, lags)


def kappa(v, L):
    """max over rows of rms_k |V[k]| / min_k |V[k]|, V = fft(v, L): the condition of the phase transform on these rows"""
    a = np.abs(np.fft.fft(np.asarray(v, dtype=np.float64 if np.dtype(v.dtype).kind != "c" else np.complex128), L, axis=-1))
    return float(np.max(np.sqrt(np.mean(a * a, axis=-1)) / np.min(a, axis=-1)))


def window_err(got, want_full, lag_first, lags):
    """||got - window(want)||_2 / ||want over all L lags||_2: rigorous for any window, rel_l2 when lags == L"""
    w = window(want_full, lag_first, lags)
    return float(np.linalg.norm(np.asarray(got, dtype=w.dtype) - w) / np.linalg.norm(want_full))
