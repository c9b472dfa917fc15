"""The truth of the N-D convolution handle (fourier_hip_convnd_*): numpy rfftn / irfftn in f64 on the inputs as rounded to the
handle's type, over the transform shape S; and scipy.signal.convolve / correlate with method="direct" for the linear modes.
No torch, no GPU."""
import numpy as np


def circular(x, h, shape, correlate=False, filter_first=0):
    """x: (B,) + in_shape, h: (F,) + k, both <= shape -> (B,) + shape in f64: item b zero-extended to `shape`, convolved circularly
    with filter (filter_first + b) mod F (correlate: with the conjugated spectrum)"""
    r = len(shape)
    axes = tuple(range(-r, 0))
    X = np.fft.rfftn(np.asarray(x, np.float64), shape, axes=axes)
    H = np.fft.rfftn(np.asarray(h, np.float64), shape, axes=axes)
    if correlate:
        H = np.conj(H)
    f = (filter_first + np.arange(x.shape[0])) % h.shape[0]
    return np.fft.irfftn(X * H[f], shape, axes=axes)


def window(y, first, size):
    """the window [first, first + size) of the trailing dimensions of y"""
    r = len(first)
    idx = (slice(None),) * (y.ndim - r) + tuple(slice(a, a + n) for a, n in zip(first, size))
    return np.ascontiguousarray(y[idx])


def linear_window(a, k, mode):
    """(first, size) of scipy.signal.convolve's `mode` in the full linear convolution of items of shape a with taps of shape k"""
    if mode == "full":
        return tuple(0 for _ in a), tuple(n + m - 1 for n, m in zip(a, k))
    if mode == "same":
        return tuple((m - 1) // 2 for m in k), tuple(a)
    return tuple(m - 1 for m in k), tuple(n - m + 1 for n, m in zip(a, k))


def scipy_linear(x, h, mode, correlate=False):
    """scipy.signal.convolve (correlate) of every item of x: (B,) + a with filter b mod F of h: (F,) + k, method="direct", in f64"""
    import scipy.signal

    fn = scipy.signal.correlate if correlate else scipy.signal.convolve
    return np.stack([fn(np.asarray(x[b], np.float64), np.asarray(h[b % h.shape[0]], np.float64), mode=mode, method="direct")
                     for b in range(x.shape[0])])
