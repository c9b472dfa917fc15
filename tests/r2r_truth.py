"""What the DCT / DST tests (test_r2r_emu.py, test_gpu_r2r.py) compare against, in numpy f64, independent of the library's route:
the dense cosine / sine matrix of scipy's definitions up to N = 256; above that, type II from the length-4N even (DCT) or odd (DST)
extension through numpy's rfft, and type III from the dense definition on sampled outputs (exact integer angle reduction)."""
import functools

import numpy as np

KINDS = {"dct2": 0, "dct3": 1, "dst2": 2, "dst3": 3}   # FOURIER_R2R_DCT2 ... DST3
NORMS = {"backward": 0, "ortho": 1, "forward": 2}      # FOURIER_R2R_NORM_*
DENSE_LIMIT = 256


def _angles(rows, cols, n):
    """pi * rows * cols / 2N for integer index arrays, reduced mod 4N before the multiplication."""
    return np.pi * ((rows[:, None].astype(np.int64) * cols[None, :].astype(np.int64)) % (4 * n)) / (2.0 * n)


def rows_of(kind, n, idx):
    """Rows `idx` of the backward-norm matrix M of a kind: output[idx] = M @ input.
      dct2  X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)          dct3  x[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)
      dst2  X[k] = 2 sum_n x[n] sin(pi (k+1) (2n+1) / 2N)      dst3  the transpose with the column of X[N-1] halved"""
    idx = np.asarray(idx, np.int64)
    full = np.arange(n, dtype=np.int64)
    if kind == "dct2":
        return 2.0 * np.cos(_angles(idx, 2 * full + 1, n))
    if kind == "dst2":
        return 2.0 * np.sin(_angles(idx + 1, 2 * full + 1, n))
    if kind == "dct3":
        m = 2.0 * np.cos(_angles(2 * idx + 1, full, n))
        m[:, 0] = 1.0
        return m
    m = 2.0 * np.sin(_angles(2 * idx + 1, full + 1, n))
    m[:, n - 1] *= 0.5
    return m


@functools.lru_cache(maxsize=None)
def dense(kind, n):
    return rows_of(kind, n, np.arange(n))


def sample_indices(n, count=None):
    """The ends, the middle and a fixed random set of output indices (fewer for a long row: each costs N cosines per input row)."""
    fixed = [0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 3, n - 2, n - 1]
    rng = np.random.default_rng(n)
    count = count or (48 if n <= 1 << 17 else 6)
    return np.unique(np.clip(np.concatenate([fixed, rng.integers(0, n, count)]), 0, n - 1))


def type2_by_extension(kind, x):
    """DCT-II / DST-II of the rows of x from the rfft of the length-4N extension y[2n+1] = x[n], y[4N-2n-1] = +-x[n]."""
    n = x.shape[-1]
    y = np.zeros(x.shape[:-1] + (4 * n,))
    y[..., 1:2 * n:2] = x
    y[..., 4 * n - 1:2 * n:-2] = x if kind == "dct2" else -x
    Y = np.fft.rfft(y, axis=-1)
    return Y.real[..., :n] if kind == "dct2" else -Y.imag[..., 1:n + 1]


def want(kind, norm, x):
    """(idx, values): the transform of the rows of x (f64) at output indices idx -- all of them, or sample_indices(N) for a type III
    above DENSE_LIMIT -- in scipy's norm: backward 1, forward 1/2N, ortho 1/sqrt(2N) with the edge element (DCT: 0, DST: N-1) of the
    transform side times 1/sqrt 2 (type II, an output) or sqrt 2 (type III, an input)."""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    edge = 0 if kind.startswith("dct") else n - 1
    type3 = kind.endswith("3")
    if type3 and norm == "ortho":
        x = x.copy()
        x[..., edge] *= np.sqrt(2.0)
    if n <= DENSE_LIMIT:
        idx, y = np.arange(n), x @ dense(kind, n).T
    elif type3:
        idx = sample_indices(n)
        y = x @ rows_of(kind, n, idx).T
    else:
        idx, y = np.arange(n), type2_by_extension(kind, x)
    if norm == "forward":
        y = y / (2.0 * n)
    elif norm == "ortho":
        y = y / np.sqrt(2.0 * n)
        if not type3:
            y[..., edge] /= np.sqrt(2.0)
    return idx, y
