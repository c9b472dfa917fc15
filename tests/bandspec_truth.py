"""f64 numpy truth of the band-spectrogram tests (tests/test_bandspec_emu.py, tests/test_gpu_bandspec.py, tests/test_mel_filterbank.py),
built on tests/spectrogram_truth.py: spectrogram(...) @ W.T with the optional log_mult * log(maximum(., floor)); an independent
restatement of the mel formulas of fourier_amd.mel_filterbank (loops over bands and bins, not the broadcast form the package uses); the
dB scaling of fourier_amd.mel_spectrogram; a DCT-II by explicit cosine matrix for the MFCC check.  No torch FFT, no GPU, no scipy."""
import math

import numpy as np

import spectrogram_truth
from spectrogram_truth import frames, hann  # noqa: F401


def band_spectrogram(x, W, n_fft, hop, win_length=None, window=None, pad_mode="reflect", power=2, normalized=False, log_mult=0.0,
                     log_floor=0.0):
    """x: (batch, length), W: (bands, bins) -> (batch, frames, bands) float64."""
    S = spectrogram_truth.spectrogram(x, n_fft, hop, win_length, window, pad_mode, power, normalized)
    Y = S @ np.asarray(W, np.float64).T
    return log_mult * np.log(np.maximum(Y, log_floor)) if log_mult != 0 else Y


def abs_band_spectrogram(x, W, n_fft, hop, win_length=None, window=None, pad_mode="reflect", power=2, normalized=False):
    """|W| @ S: the scale of a band's terms, what an error bound of a signed bank is taken against."""
    return band_spectrogram(x, np.abs(np.asarray(W, np.float64)), n_fft, hop, win_length, window, pad_mode, power, normalized)


def hz_to_mel(f, mel_scale="htk"):
    f = float(f)
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    if f < 1000.0:
        return f / (200.0 / 3.0)
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m, mel_scale="htk"):
    m = float(m)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if m < 15.0:
        return m * (200.0 / 3.0)
    return 1000.0 * math.exp((m - 15.0) * (math.log(6.4) / 27.0))


def mel_points(f_min, f_max, n_mels, mel_scale="htk"):
    """the n_mels + 2 corner frequencies f_pts, Hz"""
    m0, m1 = hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale)
    return np.array([mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), mel_scale) for i in range(n_mels + 2)])


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    f_pts = mel_points(f_min, f_max, n_mels, mel_scale)
    W = np.zeros((n_mels, n_freqs))
    for j in range(n_mels):
        for k in range(n_freqs):
            f = k * (sample_rate / 2.0) / (n_freqs - 1)
            up = (f - f_pts[j]) / (f_pts[j + 1] - f_pts[j])
            down = (f_pts[j + 2] - f) / (f_pts[j + 2] - f_pts[j + 1])
            W[j, k] = max(0.0, min(up, down))
        if norm == "slaney":
            W[j] *= 2.0 / (f_pts[j + 2] - f_pts[j])
    return W


def to_db(Y, power=2, amin=1e-10, ref=1.0, top_db=None):
    """(10 if power == 2 else 20) * log10(max(Y, amin) / ref); top_db: nothing below each leading item's maximum minus top_db"""
    d = (10.0 if power == 2 else 20.0) * np.log10(np.maximum(Y, amin) / ref)
    if top_db is not None:
        d = np.maximum(d, d.max(axis=(-2, -1), keepdims=True) - top_db)
    return d


def dct2(y, norm="ortho"):
    """scipy.fft.dct(y, 2, norm=norm) along the last axis by the explicit cosine matrix"""
    n = y.shape[-1]
    k, m = np.arange(n)[:, None], np.arange(n)[None, :]
    C = 2.0 * np.cos(np.pi * k * (2 * m + 1) / (2.0 * n))
    if norm == "ortho":
        C *= np.where(k == 0, math.sqrt(1.0 / (4.0 * n)), math.sqrt(1.0 / (2.0 * n)))
    return y @ C.T
