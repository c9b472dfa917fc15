"""f64 numpy truth of the STFT tests (tests/test_stft_emu.py, tests/test_gpu_stft.py): explicit framing with np.pad, np.fft.rfft /
np.fft.irfft and the overlap-add formula of include/fourier.h, on the rounded input.  No torch FFT, no GPU.  Frame-major: a row's
spectrogram has shape (frames, bins)."""
import numpy as np

PAD = {"none": None, "reflect": "reflect", "constant": "constant"}


def padding(n_fft, pad_mode):
    return 0 if pad_mode == "none" else n_fft // 2


def frames(length, n_fft, hop, pad_mode):
    """The frame count of a row of `length` reals, 0 where the length is invalid (torch's rules)."""
    if pad_mode == "none":
        return 1 + (length - n_fft) // hop if length >= n_fft else 0
    if length < 1 or (pad_mode == "reflect" and length <= n_fft // 2):
        return 0
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop  # even n_fft: 1 + length // hop


def full_window(window, n_fft, win_length):
    """`window` (None: ones) of win_length values centred in n_fft, f64."""
    w = np.ones(win_length) if window is None else np.asarray(window, np.float64)
    assert w.shape == (win_length,)
    left = (n_fft - win_length) // 2
    return np.concatenate([np.zeros(left), w, np.zeros(n_fft - win_length - left)])


def stft(x, n_fft, hop, win_length=None, window=None, pad_mode="reflect", normalized=False):
    """x: (batch, length) -> (batch, frames, bins) complex128."""
    x = np.asarray(x, np.float64)
    win_length = n_fft if win_length is None else win_length
    w = full_window(window, n_fft, win_length)
    p = padding(n_fft, pad_mode)
    nf = frames(x.shape[-1], n_fft, hop, pad_mode)
    assert nf > 0
    xp = x if p == 0 else np.pad(x, ((0, 0), (p, p)), mode=PAD[pad_mode])
    fr = np.stack([xp[:, f * hop:f * hop + n_fft] for f in range(nf)], axis=1) * w
    X = np.fft.rfft(fr, n=n_fft, axis=-1)
    return X / np.sqrt(n_fft) if normalized else X


def envelope(n_fft, hop, nframes, length, win_length=None, window=None, pad_mode="reflect"):
    """sum_f w[t + p - f hop]^2 for t < length."""
    win_length = n_fft if win_length is None else win_length
    w = full_window(window, n_fft, win_length)
    p = padding(n_fft, pad_mode)
    env = np.zeros(hop * (nframes - 1) + n_fft)
    for f in range(nframes):
        env[f * hop:f * hop + n_fft] += w * w
    return env[p:p + length]


def istft(X, n_fft, hop, length=None, win_length=None, window=None, pad_mode="reflect", normalized=False):
    """X: (batch, frames, bins) -> (batch, length) float64, the overlap-add over the envelope."""
    X = np.asarray(X, np.complex128)
    win_length = n_fft if win_length is None else win_length
    w = full_window(window, n_fft, win_length)
    p = padding(n_fft, pad_mode)
    nf = X.shape[1]
    full = hop * (nf - 1) + n_fft - 2 * p
    length = full if length is None else length
    assert 1 <= length <= full
    X = X.copy()
    X[..., 0] = X[..., 0].real  # irfft ignores the imaginary parts of bins 0 and n_fft / 2
    if n_fft % 2 == 0:
        X[..., -1] = X[..., -1].real
    fr = np.fft.irfft(X, n=n_fft, axis=-1) * w
    if normalized:
        fr = fr * np.sqrt(n_fft)
    y = np.zeros((X.shape[0], hop * (nf - 1) + n_fft))
    for f in range(nf):
        y[:, f * hop:f * hop + n_fft] += fr[:, f]
    return y[:, p:p + length] / envelope(n_fft, hop, nf, length, win_length, window, pad_mode)


def hann(n, dtype=np.float64):
    """The periodic Hann window (torch.hann_window's default), rounded to dtype."""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(dtype)
