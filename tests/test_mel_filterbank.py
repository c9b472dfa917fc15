"""fourier_amd.mel_filterbank on the CPU, without the library: known values of the two mel scales, the partition of unity of the
unnormalised triangles, contiguous supports, unit area under norm="slaney", no empty row at the shapes the other tests use, and
agreement with the independent restatement of tests/bandspec_truth.py."""
import numpy as np
import pytest

import bandspec_truth as truth

# (n_freqs, sample_rate, n_mels, mel_scale)
SHAPES = [(129, 16000.0, 40, "htk"), (65, 8000.0, 12, "slaney"), (1025, 48000.0, 128, "slaney"), (201, 16000.0, 40, "htk")]


@pytest.fixture(scope="module")
def mel():
    from fourier_amd.fft import mel_filterbank  # (the module binds the library lazily: no libfourier.so is loaded here)

    return mel_filterbank


def test_known_values_of_the_mel_scales():
    from fourier_amd import fft

    assert abs(float(fft._hz_to_mel(1000.0, "htk")) - 999.9855) < 1e-3
    assert abs(float(fft._hz_to_mel(1000.0, "htk")) - 2595.0 * np.log10(1.0 + 1000.0 / 700.0)) < 1e-12
    assert abs(float(fft._hz_to_mel(1000.0, "slaney")) - 15.0) < 1e-12
    assert abs(float(fft._hz_to_mel(6400.0, "slaney")) - 42.0) < 1e-12
    assert abs(float(fft._hz_to_mel(500.0, "slaney")) - 7.5) < 1e-12
    for scale in ("htk", "slaney"):
        for f in (0.0, 30.0, 999.0, 1000.0, 1001.0, 7000.0, 22050.0):
            assert abs(float(fft._mel_to_hz(fft._hz_to_mel(f, scale), scale)) - f) <= 1e-9 * max(f, 1.0)
            assert abs(float(fft._hz_to_mel(f, scale)) - truth.hz_to_mel(f, scale)) <= 1e-12 * max(truth.hz_to_mel(f, scale), 1.0)


@pytest.mark.parametrize("n_freqs,sr,n_mels,scale", SHAPES)
def test_partition_of_unity_supports_and_rows(mel, n_freqs, sr, n_mels, scale):
    W = mel(n_freqs, 0.0, sr / 2, n_mels, sr, None, scale)
    assert W.shape == (n_mels, n_freqs) and W.dtype == np.float64
    assert np.all(W >= 0) and np.all(W <= 1 + 1e-15)
    f_pts = truth.mel_points(0.0, sr / 2, n_mels, scale)
    freqs = np.linspace(0.0, sr / 2, n_freqs)
    inside = (freqs >= f_pts[1]) & (freqs <= f_pts[n_mels])
    assert inside.sum() > 0
    assert np.max(np.abs(W[:, inside].sum(axis=0) - 1.0)) <= 1e-12  # between the first and the last peak the triangles sum to 1
    for j in range(n_mels):
        nz = np.flatnonzero(W[j])
        assert nz.size > 0, (j, "an empty row")
        assert nz[-1] - nz[0] + 1 == nz.size, (j, "the support is not one run")
        assert freqs[nz[0]] > f_pts[j] and freqs[nz[-1]] < f_pts[j + 2]


@pytest.mark.parametrize("n_freqs,sr,n_mels,scale", SHAPES)
def test_agrees_with_the_restatement(mel, n_freqs, sr, n_mels, scale):
    for norm in (None, "slaney"):
        for f_min, f_max in ((0.0, sr / 2), (20.0, 0.45 * sr)):
            got = mel(n_freqs, f_min, f_max, n_mels, sr, norm, scale)
            want = truth.mel_filterbank(n_freqs, f_min, f_max, n_mels, sr, norm, scale)
            scale_of = max(1.0, np.abs(want).max())
            assert np.max(np.abs(got - want)) <= 1e-12 * scale_of, (norm, f_min, np.max(np.abs(got - want)))


def test_slaney_norm_gives_unit_area(mel):
    """The trapezoid rule on a grid of step d is exact for a piecewise-linear function except in the intervals that hold a kink, where
    it is off by at most d^2 / 8 times the jump of the slope.  A triangle of unit area on [f0, f1, f2], a = f1 - f0, b = f2 - f1, has
    the peak 2 / (a + b) and slope jumps that sum to 4 / (a b): the quadrature error is at most d^2 / (2 a b)."""
    sr, n_mels, n_freqs = 16000.0, 12, 16001  # a grid of 0.5 Hz
    for scale in ("htk", "slaney"):
        W = mel(n_freqs, 0.0, sr / 2, n_mels, sr, "slaney", scale)
        d = (sr / 2) / (n_freqs - 1)
        f_pts = truth.mel_points(0.0, sr / 2, n_mels, scale)
        for j in range(n_mels):
            area = d * (W[j].sum() - 0.5 * (W[j, 0] + W[j, -1]))
            a, b = f_pts[j + 1] - f_pts[j], f_pts[j + 2] - f_pts[j + 1]
            assert abs(area - 1.0) <= d * d / (2 * a * b) + 1e-12, (scale, j, area)


def test_argument_errors(mel):
    with pytest.raises(ValueError):
        mel(129, 0.0, 8000.0, 40, 16000.0, norm="area")
    with pytest.raises(ValueError):
        mel(129, 0.0, 8000.0, 40, 16000.0, mel_scale="bark")
    with pytest.raises(ValueError):
        mel(129, 4000.0, 4000.0, 40, 16000.0)
    with pytest.raises(ValueError):
        mel(1, 0.0, 8000.0, 40, 16000.0)
    with pytest.raises(ValueError):
        mel(129, 0.0, 8000.0, 0, 16000.0)
