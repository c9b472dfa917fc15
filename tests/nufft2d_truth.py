"""The truth of the 2-D non-uniform FFT handle (fourier_hip_nufft2d_*): the direct sums in f64 on the inputs as rounded to the handle's
type (the phases k_d x_d,j are formed and reduced modulo 2 pi in long double per axis, tests/nufft_truth.py's phases), and a numpy
model of the handle's algorithm (include/fourier.h) that runs in f64 or in the handle's type T: the second gives the rounding term
of the bounds in tests/nufft2d_cases.py.  Width, grid length, mode order and the quadrature of phihat are the 1-D truth's.  No torch,
no GPU."""
import numpy as np
import scipy.fft

from nufft_truth import cdt, grid_length, mode_indices, phases, phihat, rdt, width  # noqa: F401


def direct_modes(x1, x2, c, n, sign, order=0):
    """type 1: f[b, k1, k2] = sum_j c[b, j] exp(i sign (k1 x1_j + k2 x2_j)); c: (B, M) -> (B, n1, n2) in f64"""
    c = np.asarray(c, np.complex128)
    out = np.zeros((c.shape[0], n[0], n[1]), np.complex128)
    if len(x1):
        p1, p2 = phases(x1, mode_indices(n[0], order), sign), phases(x2, mode_indices(n[1], order), sign)
        for b in range(c.shape[0]):
            out[b] = (p1 * c[b][:, None]).T @ p2
    return out


def direct_points(x1, x2, f, sign, order=0):
    """type 2: c[b, j] = sum_{k1,k2} f[b, k1, k2] exp(i sign (k1 x1_j + k2 x2_j)); f: (B, n1, n2) -> (B, M) in f64"""
    f = np.asarray(f, np.complex128)
    out = np.zeros((f.shape[0], len(x1)), np.complex128)
    if len(x1):
        p1, p2 = phases(x1, mode_indices(f.shape[1], order), sign), phases(x2, mode_indices(f.shape[2], order), sign)
        for b in range(f.shape[0]):
            out[b] = ((p1 @ f[b]) * p2).sum(axis=1)
    return out


class Axis:
    """one axis of the model: the cells and the weights of every point, and the deconvolution factor of every mode"""

    def __init__(self, n, w, x, T):
        self.L = L = grid_length(n, w)
        x = np.asarray(x, np.float64)
        xf = x - 2 * np.pi * np.floor(x / (2 * np.pi))
        g = xf * (L / (2 * np.pi))
        self.g = g = np.where(g >= L, g - L, g)
        c = np.ceil(g - w / 2)
        self.i0 = c.astype(np.int64)
        d = (c - g).astype(T)
        beta, ihw = T(2.30 * w), T(2) / T(w)
        z = (d[:, None] + np.arange(w).astype(T)[None, :]) * ihw
        q = T(1) - z * z
        self.wt = np.exp(beta * (np.sqrt(np.maximum(q, T(0))) - T(1))).astype(T)  # [p, t]
        self.cells = (self.i0[:, None] + np.arange(w)[None, :]) % L
        k = mode_indices(n, 0)
        self.cell_of_k = np.where(k < 0, k + L, k)
        self.inv_of_k = (1.0 / phihat(w, L, np.arange(n // 2 + 1))).astype(T)[np.abs(k)]


class Model:
    """the handle's algorithm in numpy for n = (n1, n2) modes, accuracy eps and points (x1, x2); real = the handle's precision (it
    sets the clamp of w), arith = "f64" or the handle's precision: the type the weights, the grid, the transforms and the factors
    are held in"""

    def __init__(self, n, eps, x1, x2, real, arith="f64"):
        self.n, self.real, self.arith = tuple(n), real, arith
        self.w = w = width(eps, real)
        T = rdt(arith)
        self.a1, self.a2 = Axis(n[0], w, x1, T), Axis(n[1], w, x2, T)
        self.L = (self.a1.L, self.a2.L)
        self.m = len(np.asarray(x1))
        self.inv = (self.a1.inv_of_k[:, None] * self.a2.inv_of_k[None, :]).astype(T)

    def _fft(self, g, sign):
        return scipy.fft.fft2(g, axes=(-2, -1)) if sign < 0 else scipy.fft.ifft2(g, axes=(-2, -1), norm="forward")

    def to_modes(self, c, sign, order=0):
        C = cdt(self.arith)
        c = np.asarray(c).astype(C)
        L1, L2 = self.L
        g = np.zeros((c.shape[0], L1 * L2), C)
        for t1 in range(self.w if self.m else 0):
            for t2 in range(self.w):
                wt = (self.a1.wt[:, t1] * self.a2.wt[:, t2])
                np.add.at(g, (slice(None), self.a1.cells[:, t1] * L2 + self.a2.cells[:, t2]), wt[None, :] * c)
        g = self._fft(g.reshape(-1, L1, L2), sign).astype(C)
        f = (g[:, self.a1.cell_of_k[:, None], self.a2.cell_of_k[None, :]] * self.inv[None]).astype(C)
        return f if order == 0 else np.fft.ifftshift(f, axes=(-2, -1))

    def to_points(self, f, sign, order=0):
        C = cdt(self.arith)
        f = np.asarray(f).astype(C)
        if order == 1:
            f = np.fft.fftshift(f, axes=(-2, -1))
        L1, L2 = self.L
        g = np.zeros((f.shape[0], L1, L2), C)
        g[:, self.a1.cell_of_k[:, None], self.a2.cell_of_k[None, :]] = f * self.inv[None]
        g = self._fft(g, sign).astype(C).reshape(-1, L1 * L2)
        acc = np.zeros((f.shape[0], self.m), C)
        for t1 in range(self.w if self.m else 0):
            for t2 in range(self.w):
                wt = (self.a1.wt[:, t1] * self.a2.wt[:, t2])
                acc = (acc + wt[None, :] * g[:, self.a1.cells[:, t1] * L2 + self.a2.cells[:, t2]]).astype(C)
        return acc
