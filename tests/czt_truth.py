"""f64 truth of the chirp-z tests (tests/test_czt_emu.py, tests/test_gpu_czt.py): the definition of include/fourier.h as a direct sum on
the rounded input,

    X[b, k] = sum_{j<n} x[b, j] a^-j w^(j k),   w = w_abs exp(2 pi i w_turns),  a = a_abs exp(2 pi i a_turns),

with every phase frac(w_turns j k - a_turns j) computed from the double parameters by exact integer arithmetic (fractions.Fraction on
Python ints: a double is a dyadic rational; `phases` explains where the vectorised form rounds), and every magnitude as exp(log(w_abs) j k - log(a_abs) j).  scipy.signal.czt is not the truth: its
w**(k**2/2) is 2e-12 off at n = 100 already.  No FFT, no torch, no GPU."""
import functools
from fractions import Fraction

import numpy as np


def rows(rng, batch, n, dtype):
    """seeded white Gaussian rows, rounded to `dtype` (a complex dtype: both parts Gaussian)"""
    dtype = np.dtype(dtype)
    x = rng.standard_normal((batch, n))
    if dtype.kind == "c":
        x = x + 1j * rng.standard_normal((batch, n))
    return np.ascontiguousarray(x.astype(dtype))


def exact_phases(n, bins, w_turns, a_turns):
    """frac(w_turns j k - a_turns j) for j < n, k in bins, by exact integer arithmetic on Python ints (object arrays) and ONE correctly
    rounded division per phase: what _kernel's fast path is checked against (tests/test_czt_emu.py)"""
    wn, wd = Fraction(w_turns).as_integer_ratio()
    an, ad = Fraction(a_turns).as_integer_ratio()
    den = wd * ad  # a power of two
    j = np.arange(n, dtype=object)[:, None]
    k = np.array(bins, dtype=object)[None, :]
    return ((((wn * ad) * j) * k - (an * wd) * j) % den / den).astype(np.float64)


HI_BITS = 36  # of w_turns j: its product with a bin below 2^16 is exact in f64


def phases(n, bins, w_turns, a_turns):
    """The same phases (modulo whole turns) in vectorised f64, 10 x faster.  Per row j, exact on Python ints: r_j = frac(w_turns j) and
    c_j = frac(a_turns j) (a double is a dyadic rational).  r_j is split into its leading HI_BITS bits hi_j and the rest lo_j < 2^-36,
    each one correctly rounded division; hi_j k is then exact in f64 for k < 2^16 and so is its fraction, lo_j k < 2^-20 carries a
    relative 2^-53, and the two additions round once each: within 3.5e-16 of a turn of the exact value, where f64 itself resolves
    1.1e-16."""
    wn, wd = Fraction(w_turns).as_integer_ratio()
    an, ad = Fraction(a_turns).as_integer_ratio()
    assert max(bins) < 1 << 16
    shift = max(wd.bit_length() - 1 - HI_BITS, 0)
    r = [(wn * j) % wd for j in range(n)]
    hi = np.array([(v >> shift) / (wd >> shift) for v in r])          # exact: at most HI_BITS bits
    lo = np.array([(v & ((1 << shift) - 1)) / wd for v in r])        # correctly rounded
    c = np.array([((an * j) % ad) / ad for j in range(n)])           # correctly rounded
    k = np.asarray(bins, dtype=np.float64)[None, :]
    t = hi[:, None] * k
    t -= np.floor(t)
    return t + lo[:, None] * k - c[:, None]


@functools.lru_cache(maxsize=4)
def _kernel(n, bins, w_abs, w_turns, a_abs, a_turns):
    jf = np.arange(n, dtype=np.float64)[:, None]
    kf = np.asarray(bins, dtype=np.float64)[None, :]
    mag = np.exp(np.log(w_abs) * (jf * kf) - np.log(a_abs) * jf)
    ang = 2.0 * np.pi * phases(n, bins, w_turns, a_turns)
    return mag * (np.cos(ang) + 1j * np.sin(ang))


def kernel(n, bins, w_abs, w_turns, a_abs, a_turns):
    """K[j, i] = a^-j w^(j bins[i]) as complex128, phases exact; the last few are kept, so that the precisions of a case share one"""
    return _kernel(int(n), tuple(int(k) for k in bins), float(w_abs), float(w_turns), float(a_abs), float(a_turns))


def czt(x, m, w_abs, w_turns, a_abs=1.0, a_turns=0.0, bins=None):
    """x: (batch, n) -> (batch, m) complex128, or (batch, len(bins)) for a subset of the bins"""
    x = np.asarray(x)
    x = x.astype(np.complex128)
    bins = range(m) if bins is None else bins
    return x @ kernel(x.shape[-1], bins, w_abs, w_turns, a_abs, a_turns)


def chirp_ratio(n, m, w_abs, a_abs):
    """R: the largest over the smallest magnitude among A[j] = a_abs^-j w_abs^(j^2/2), j < n, and B[k] = w_abs^(k^2/2), k < m"""
    j = np.arange(n, dtype=np.float64)
    k = np.arange(m, dtype=np.float64)
    logs = np.concatenate([np.log(float(w_abs)) * j * j / 2 - np.log(float(a_abs)) * j, np.log(float(w_abs)) * k * k / 2])
    return float(np.exp(logs.max() - logs.min()))
