"""f64 numpy truth of the cross-spectrum tests (tests/test_csd_emu.py, tests/test_gpu_csd.py), built on tests/stft_truth.py: the formulas
of include/fourier.h, scale * c_k / frames * sum_f conj(X) Y and |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2) with the unnormalized
frames X of x and Y of y, in f64 on the rounded input.  No torch FFT, no GPU.

pair() makes the inputs of every accuracy check: x white Gaussian, y = 0.6 roll(x, 5) + 0.8 independent white Gaussian, so |Pxy| stays
near 0.6 sqrt(Pxx Pyy) and no bin is near zero in norm (independent x and y would make Pxy a cancelling sum whose relative error grows
with the square root of the frame count)."""
import numpy as np

import stft_truth
from spectrogram_truth import fold_factors, welch_scale  # noqa: F401
from stft_truth import frames, hann  # noqa: F401


def pair(rng, batch, length, dtype):
    x = rng.standard_normal((batch, length))
    y = 0.6 * np.roll(x, 5, axis=-1) + 0.8 * rng.standard_normal((batch, length))
    return np.ascontiguousarray(x.astype(dtype)), np.ascontiguousarray(y.astype(dtype))


def _sums(x, y, n_fft, hop, win_length, window, pad_mode):
    X = stft_truth.stft(x, n_fft, hop, win_length, window, pad_mode, False)
    Y = stft_truth.stft(y, n_fft, hop, win_length, window, pad_mode, False)
    return (np.conj(X) * Y).sum(axis=1), (X.real ** 2 + X.imag ** 2).sum(axis=1), (Y.real ** 2 + Y.imag ** 2).sum(axis=1), X.shape[1]


def csd(x, y, n_fft, hop, win_length=None, window=None, pad_mode="none", onesided_fold=True, scale=1.0):
    """x, y: (batch, length) -> (batch, bins) complex128."""
    pxy, _, _, nf = _sums(x, y, n_fft, hop, win_length, window, pad_mode)
    return scale * (fold_factors(n_fft) if onesided_fold else 1.0) * pxy / nf


def coherence(x, y, n_fft, hop, win_length=None, window=None, pad_mode="none"):
    """x, y: (batch, length) -> (batch, bins) float64."""
    pxy, pxx, pyy, _ = _sums(x, y, n_fft, hop, win_length, window, pad_mode)
    return (pxy.real ** 2 + pxy.imag ** 2) / (pxx * pyy)
