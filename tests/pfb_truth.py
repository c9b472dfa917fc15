"""The truth of the polyphase filter bank tests (tests/test_pfb_emu.py, tests/test_gpu_pfb.py): f64 numpy on the rounded input.

    frames(length) = 1 + (length - P T) / D  for length >= P T, else 0
    u[f, n] = sum_{t < T} h[t P + n] x[f D + t P + n]
    X[f, k] = sum_{n < P} u[f, n] exp(-2 pi i k n / P)          (real rows: k <= P / 2)

pfb() folds and transforms; pfb_by_long_dft() is the independent statement the module checks it against when run as a program (and
tests/test_pfb_emu.py once): X[f, k] is bin T k of the P T-point DFT of the windowed frame, since exp(-2 pi i (T k)(t P + n) / (P T)) =
exp(-2 pi i k n / P).  The two agree to 3e-16 relative L2."""
import numpy as np


def frames(length, P, T, D):
    return 1 + (length - P * T) // D if length >= P * T else 0


def windowed_frames(x, h, P, T, D):
    """(batch, frames, P T): every frame's values times the filter, f64"""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    nf = frames(x.shape[-1], P, T, D)
    assert nf > 0
    idx = D * np.arange(nf)[:, None] + np.arange(P * T)[None, :]
    return x[:, idx] * np.asarray(h, np.float64).reshape(1, 1, P * T)


def pfb(x, h, P, T, D, real_input):
    """x: (batch, length) rounded input, h: P T reals (None: ones) -> (batch, frames, bins) complex128"""
    h = np.ones(P * T) if h is None else h
    w = windowed_frames(x, h, P, T, D)
    u = w.reshape(w.shape[0], w.shape[1], T, P).sum(axis=2)
    return np.fft.rfft(u, axis=-1) if real_input else np.fft.fft(u, axis=-1)


def pfb_by_long_dft(x, h, P, T, D, real_input):
    h = np.ones(P * T) if h is None else h
    X = np.fft.fft(windowed_frames(x, h, P, T, D), axis=-1)[..., ::T]
    return X[..., : P // 2 + 1] if real_input else X


def fold_in_precision(x, h, P, T, D, real_input):
    """The restatement the tolerance is measured with: the fold in the input's own precision, taps in the order t = 0, 1, ..., then an
    exact (f64) DFT.  Its distance from pfb() is the rounding the tap sum adds."""
    x = np.asarray(x)
    nf = frames(x.shape[-1], P, T, D)
    idx = D * np.arange(nf)[:, None] + np.arange(P * T)[None, :]
    w = (x[:, idx] * np.asarray(h, x.real.dtype).reshape(1, 1, P * T)).reshape(x.shape[0], nf, T, P)
    u = w[:, :, 0]
    for t in range(1, T):
        u = u + w[:, :, t]
    u = u.astype(np.complex128 if np.iscomplexobj(u) else np.float64)
    return np.fft.rfft(u, axis=-1) if real_input else np.fft.fft(u, axis=-1)


def self_check():
    rng = np.random.default_rng(0)
    worst = 0.0
    for P, T, D, real_input in ((16, 3, 5, True), (16, 4, 16, False), (9, 2, 4, True), (12, 8, 9, False)):
        length = P * T + 3 * D + 1
        x = rng.standard_normal((2, length)) + (0 if real_input else 1j * rng.standard_normal((2, length)))
        h = 0.5 + rng.random(P * T)
        a, b = pfb(x, h, P, T, D, real_input), pfb_by_long_dft(x, h, P, T, D, real_input)
        worst = max(worst, float(np.linalg.norm(a - b) / np.linalg.norm(a)))
    return worst


if __name__ == "__main__":
    print(self_check())
