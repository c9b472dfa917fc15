"""f64 numpy truth of the MDCT tests (tests/test_mdct_emu.py, tests/test_gpu_mdct.py): the dense cosine matrix of the definition in
include/fourier.h on the rounded input, explicit framing and zero padding, the inverse by the dense transpose plus overlap-add.
Independent of every route of the library: no fold, no FFT.  A frame is 2n samples, the hop n; a row's coefficients have shape
(frames, n)."""
import numpy as np


def frames(length, n, center=True):
    """The frame count of a row of `length` reals, 0 where the length is invalid."""
    if center:
        return -(-length // n) + 1 if length >= 1 else 0
    return length // n - 1 if length >= 2 * n else 0


def default_length(nframes, n, center=True):
    """The longest row `nframes` frames give back."""
    return (nframes - 1) * n if center else (nframes + 1) * n


def sine_window(n, dtype=np.float64):
    """The default window sin(pi (m + 1/2) / 2n), m < 2n, rounded to dtype."""
    return np.sin(np.pi * (np.arange(2 * n) + 0.5) / (2 * n)).astype(dtype)


def princen_bradley_window(rng, n, dtype=np.float64):
    """A random window with w[m]^2 + w[m + n]^2 = 1 and w[m] = w[2n - 1 - m], rounded to dtype."""
    theta = rng.uniform(0.1, np.pi / 2 - 0.1, n)
    theta = np.concatenate([theta[: n // 2], (np.pi / 4) * np.ones(n % 2), np.pi / 2 - theta[: n // 2][::-1]])  # theta[m] + theta[n-1-m] = pi/2
    rise = np.sin(theta)
    return np.concatenate([rise, rise[::-1]]).astype(dtype)


def cosines(n):
    """C[m, k] = cos(pi/n (m + 1/2 + n/2)(k + 1/2)), shape (2n, n).  The angle is pi / 4n times (2m + 1 + n)(2k + 1), reduced mod 8n as
    integers before the multiplication."""
    m = np.arange(2 * n, dtype=np.int64)[:, None]
    k = np.arange(n, dtype=np.int64)[None, :]
    return np.cos(((2 * m + 1 + n) * (2 * k + 1) % (8 * n)).astype(np.float64) * (np.pi / (4 * n)))


def _window(window, n):
    w = sine_window(n) if window is None else np.asarray(window, np.float64)
    assert w.shape == (2 * n,)
    return w


def mdct(x, n, window=None, center=True, normalized=False):
    """x: (batch, length) -> (batch, frames, n) float64."""
    x = np.asarray(x, np.float64)
    w = _window(window, n)
    length = x.shape[-1]
    nf = frames(length, n, center)
    assert nf > 0
    p = n if center else 0
    total = (nf + 1) * n
    xp = np.zeros((x.shape[0], max(total, p + length)))
    xp[:, p:p + length] = x
    fr = np.stack([xp[:, f * n:f * n + 2 * n] for f in range(nf)], axis=1) * w
    X = fr @ cosines(n)
    return X * np.sqrt(2.0 / n) if normalized else X


def imdct(X, n, length=None, window=None, center=True, normalized=False):
    """X: (batch, frames, n) -> (batch, length) float64: the dense transpose, the window and the sum of the frames that cover a sample,
    times 2 / n (sqrt(2 / n) where normalized).  No envelope division."""
    X = np.asarray(X, np.float64)
    w = _window(window, n)
    nf = X.shape[1]
    full = default_length(nf, n, center)
    length = full if length is None else length
    assert 1 <= length <= full
    p = n if center else 0
    Y = (X @ cosines(n).T) * w
    y = np.zeros((X.shape[0], (nf + 1) * n))
    for f in range(nf):
        y[:, f * n:f * n + 2 * n] += Y[:, f]
    return y[:, p:p + length] * (np.sqrt(2.0 / n) if normalized else 2.0 / n)
