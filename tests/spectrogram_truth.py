"""f64 numpy truth of the spectrogram tests (tests/test_spectrogram_emu.py, tests/test_gpu_spectrogram.py), built on tests/stft_truth.py:
np.abs(stft(...)) ** p, and the Welch formula of include/fourier.h, scale * c_k / frames * sum_f |X|^2 with the unnormalized X, in f64 on
the rounded input.  No torch FFT, no GPU."""
import numpy as np

import stft_truth
from stft_truth import frames, hann  # noqa: F401


def spectrogram(x, n_fft, hop, win_length=None, window=None, pad_mode="reflect", power=2, normalized=False):
    """x: (batch, length) -> (batch, frames, bins) float64."""
    return np.abs(stft_truth.stft(x, n_fft, hop, win_length, window, pad_mode, normalized)) ** power


def fold_factors(n_fft):
    """c_k of a one-sided fold: 2 for the bins that have a mirror, 0 < k < n_fft / 2 and k = (n_fft - 1) / 2 at odd n_fft."""
    k = np.arange(n_fft // 2 + 1)
    return np.where((k > 0) & (2 * k < n_fft), 2.0, 1.0)


def welch(x, n_fft, hop, win_length=None, window=None, pad_mode="none", onesided_fold=True, scale=1.0):
    """x: (batch, length) -> (batch, bins) float64."""
    X = stft_truth.stft(x, n_fft, hop, win_length, window, pad_mode, False)
    p = (X.real ** 2 + X.imag ** 2).sum(axis=1) / X.shape[1]
    return scale * (fold_factors(n_fft) if onesided_fold else 1.0) * p


def welch_scale(window, fs=1.0, scaling="density"):
    w = np.asarray(window, np.float64)
    return 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2
