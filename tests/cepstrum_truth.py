"""f64 numpy truth of the cepstrum tests (tests/test_cepstrum_emu.py, tests/test_gpu_cepstrum.py): the definitions of include/fourier.h
by np.fft.fft / ifft in f64 on the inputs AS ROUNDED to the handle's type.  No torch FFT, no GPU.

    X = fft(x, L),  g = log_mult ln(max(|X|, log_floor))
    CEPSTRUM       c = ifft(g) (real and even);  out = c[:m]
    MINIMUM_PHASE  chat = fold(c): weight 1 at 0, 2 for 0 < q < L/2, 1 at L/2 (even L), 0 above;  C = fft(chat),
                   h = Re ifft(exp(C));  out = h[:m]

kappa = ||x||_2 / min_k max(|X_k|, log_floor) is the condition number of the logarithm in the measures of tests/cepstrum_cases.py: from
||dX||_2 <= base ||X||_2 = base sqrt(L) ||x||_2 follows |dg_k| <= |log_mult| |dX_k| / max(|X_k|, floor) to first order, so
||dc||_2 = ||dg||_2 / sqrt(L) <= |log_mult| kappa base."""
import numpy as np

CEPSTRUM, MINIMUM_PHASE = 0, 1


def rows(rng, batch, n, dtype):
    """x[0] = 1 plus 0.2 N(0, 1) / sqrt(n) on every sample, seeded, rounded to `dtype`: |X| stays near 1, kappa small"""
    v = 0.2 * rng.standard_normal((batch, n)) / np.sqrt(n)
    v[:, 0] += 1.0
    return np.ascontiguousarray(v.astype(dtype))


def spectrum(x, L):
    return np.fft.fft(np.asarray(x).astype(np.float64), L, axis=-1)


def log_spectrum(x, L, log_mult=1.0, log_floor=0.0):
    with np.errstate(divide="ignore"):
        return log_mult * np.log(np.maximum(np.abs(spectrum(x, L)), log_floor))


def fold_weights(L):
    w = np.zeros(L)
    w[0] = 1.0
    w[1:(L + 1) // 2] = 2.0
    if L % 2 == 0:
        w[L // 2] = 1.0
    return w


def cepstrum_full(x, L, log_mult=1.0, log_floor=0.0):
    """the whole rows of L quefrencies, f64"""
    with np.errstate(invalid="ignore"):
        return np.fft.ifft(log_spectrum(x, L, log_mult, log_floor), axis=-1).real


def folded_spectrum(x, L, log_mult=1.0, log_floor=0.0):
    """C = fft(fold(c)): its imaginary part is the phase of the minimum-phase spectrum"""
    return np.fft.fft(cepstrum_full(x, L, log_mult, log_floor) * fold_weights(L), axis=-1)


def minimum_phase_full(x, L, log_mult=1.0, log_floor=0.0):
    """the whole rows of L samples, f64"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.fft.ifft(np.exp(folded_spectrum(x, L, log_mult, log_floor)), axis=-1).real


def full(mode, x, L, log_mult=1.0, log_floor=0.0):
    return (cepstrum_full if mode == CEPSTRUM else minimum_phase_full)(x, L, log_mult, log_floor)


def kappa(x, L, log_floor=0.0):
    """per row: ||x||_2 / min_k max(|X_k|, log_floor)"""
    x = np.asarray(x).astype(np.float64)
    return np.linalg.norm(x, axis=-1) / np.maximum(np.abs(spectrum(x, L)), log_floor).min(axis=-1)


def max_phase(x, L, log_mult=1.0, log_floor=0.0):
    """max_k |Im C_k| over all rows"""
    return float(np.abs(folded_spectrum(x, L, log_mult, log_floor).imag).max())


def err(mode, got, x, L, m, log_mult=1.0, log_floor=0.0):
    """the worst row of
         CEPSTRUM       ||got - want||_2 / (|log_mult| kappa)
         MINIMUM_PHASE  ||got - want||_2 / (||h_full||_2 |log_mult| kappa),  h_full the truth's whole row of L"""
    want = full(mode, x, L, log_mult, log_floor)
    diff = np.linalg.norm(np.asarray(got).astype(np.float64) - want[:, :m], axis=-1)
    den = abs(log_mult) * kappa(x, L, log_floor)
    if mode == MINIMUM_PHASE:
        den = den * np.linalg.norm(want, axis=-1)
    return float(np.max(diff / den))
