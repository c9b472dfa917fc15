"""The truth of the 3-D non-uniform FFT handle (fourier_hip_nufft3d_*): the direct sums in f64 on the inputs as rounded to the handle's
type (the phases k_d x_d,j are formed and reduced modulo 2 pi in long double per axis, tests/nufft_truth.py's phases), and a numpy
model of the handle's algorithm (include/fourier.h) that runs in f64 or in the handle's type T: the second gives the rounding term
of the bounds in tests/nufft3d_cases.py.  Width, grid length, mode order and the quadrature of phihat are the 1-D truth's, the axis
of the model is the 2-D truth's.  No torch, no GPU."""
import numpy as np
import scipy.fft

from nufft2d_truth import Axis
from nufft_truth import cdt, grid_length, mode_indices, phases, phihat, rdt, width  # noqa: F401


def _phases(x, n, sign, order):
    return [phases(x[d], mode_indices(n[d], order), sign) for d in range(3)]  # each (M, n_d)


def direct_modes(x1, x2, x3, c, n, sign, order=0):
    """type 1: f[b, k1, k2, k3] = sum_j c[b, j] exp(i sign (k1 x1_j + k2 x2_j + k3 x3_j)); c: (B, M) -> (B, n1, n2, n3) in f64"""
    c = np.asarray(c, np.complex128)
    out = np.zeros((c.shape[0], n[0], n[1], n[2]), np.complex128)
    if len(x1):
        p1, p2, p3 = _phases((x1, x2, x3), n, sign, order)
        p23 = (p2[:, :, None] * p3[:, None, :]).reshape(len(x1), -1)  # (M, n2 n3)
        for b in range(c.shape[0]):
            out[b] = ((p1 * c[b][:, None]).T @ p23).reshape(n)
    return out


def direct_points(x1, x2, x3, f, sign, order=0):
    """type 2: c[b, j] = sum_{k1,k2,k3} f[b, k1, k2, k3] exp(i sign (k1 x1_j + k2 x2_j + k3 x3_j)); f: (B, n1, n2, n3) -> (B, M)"""
    f = np.asarray(f, np.complex128)
    out = np.zeros((f.shape[0], len(x1)), np.complex128)
    if len(x1):
        n = f.shape[1:]
        p1, p2, p3 = _phases((x1, x2, x3), n, sign, order)
        p23 = (p2[:, :, None] * p3[:, None, :]).reshape(len(x1), -1)
        for b in range(f.shape[0]):
            out[b] = ((p1 @ f[b].reshape(n[0], -1)) * p23).sum(axis=1)
    return out


class Model:
    """the handle's algorithm in numpy for n = (n1, n2, n3) modes, accuracy eps and points (x1, x2, x3); real = the handle's precision
    (it sets the clamp of w), arith = "f64" or the handle's precision: the type the weights, the grid, the transforms and the factors
    are held in"""

    def __init__(self, n, eps, x1, x2, x3, real, arith="f64"):
        self.n, self.real, self.arith = tuple(n), real, arith
        self.w = w = width(eps, real)
        T = rdt(arith)
        self.ax = [Axis(n[d], w, x, T) for d, x in enumerate((x1, x2, x3))]
        self.L = tuple(a.L for a in self.ax)
        self.m = len(np.asarray(x1))
        a1, a2, a3 = self.ax
        self.inv = ((a1.inv_of_k[:, None, None] * a2.inv_of_k[None, :, None]).astype(T) * a3.inv_of_k[None, None, :]).astype(T)
        self.pick = (a1.cell_of_k[:, None, None], a2.cell_of_k[None, :, None], a3.cell_of_k[None, None, :])

    def _fft(self, g, sign):
        return scipy.fft.fftn(g, axes=(-3, -2, -1)) if sign < 0 else scipy.fft.ifftn(g, axes=(-3, -2, -1), norm="forward")

    def _taps(self):
        """(flat cells, weights) of every point for each of the w^3 taps, axis 1 outermost"""
        a1, a2, a3 = self.ax
        L1, L2, L3 = self.L
        for t1 in range(self.w if self.m else 0):
            for t2 in range(self.w):
                w12 = a1.wt[:, t1] * a2.wt[:, t2]
                c12 = (a1.cells[:, t1] * L2 + a2.cells[:, t2]) * L3
                for t3 in range(self.w):
                    yield c12 + a3.cells[:, t3], w12 * a3.wt[:, t3]

    def to_modes(self, c, sign, order=0):
        C = cdt(self.arith)
        c = np.asarray(c).astype(C)
        g = np.zeros((c.shape[0], int(np.prod(self.L))), C)
        for cells, wt in self._taps():
            np.add.at(g, (slice(None), cells), wt[None, :] * c)
        g = self._fft(g.reshape((-1,) + self.L), sign).astype(C)
        f = (g[(slice(None),) + self.pick] * self.inv[None]).astype(C)
        return f if order == 0 else np.fft.ifftshift(f, axes=(-3, -2, -1))

    def to_points(self, f, sign, order=0):
        C = cdt(self.arith)
        f = np.asarray(f).astype(C)
        if order == 1:
            f = np.fft.fftshift(f, axes=(-3, -2, -1))
        g = np.zeros((f.shape[0],) + self.L, C)
        g[(slice(None),) + self.pick] = f * self.inv[None]
        g = self._fft(g, sign).astype(C).reshape(f.shape[0], -1)
        acc = np.zeros((f.shape[0], self.m), C)
        for cells, wt in self._taps():
            acc = (acc + wt[None, :] * g[:, cells]).astype(C)
        return acc
