"""The truth of the non-uniform FFT handle (fourier_hip_nufft_*): the direct sums in f64 on the inputs as rounded to the handle's type
(the phases k x_j are formed and reduced modulo 2 pi in long double, so that points far outside [-pi, pi) cost nothing), and a numpy
model of the handle's algorithm (include/fourier.h) that runs in f64 or in the handle's type T: the second gives the rounding term
of the bounds in tests/nufft_cases.py.  No torch, no GPU."""
import math

import numpy as np
import scipy.fft

MAX_W = {"f32": 8, "f64": 16}


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def width(eps, real):
    """w = ceil(log10(1 / eps)) + 1, clamped to 2 .. 8 at f32 and 2 .. 16 at f64"""
    return int(min(max(math.ceil(math.log10(1.0 / eps)) + 1, 2), MAX_W[real]))


def grid_length(n, w):
    """the smallest 2^a 3^b 5^c >= max(2 n, 2 w)"""
    need = max(2 * n, 2 * w)
    m = need
    while True:
        r = m
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


def mode_indices(n, order=0):
    """the mode index k of every position of a row of n modes"""
    k = np.arange(-(n // 2), n - n // 2)
    return k if order == 0 else np.fft.ifftshift(k)


def phases(x, k, sign):
    """exp(i sign k x_j) as an array [j, k], the product reduced modulo 2 pi in long double"""
    two_pi = 2 * np.arccos(np.longdouble(-1))  # pi to long double's precision; k x is exact in it for |k| < 2^11
    p = np.outer(np.asarray(x, np.longdouble), np.asarray(k, np.longdouble))
    p = (p - two_pi * np.rint(p / two_pi)).astype(np.float64)
    return np.cos(p) + (1j * sign) * np.sin(p)


def direct_modes(x, c, n, sign, order=0):
    """type 1: f[b, k] = sum_j c[b, j] exp(i sign k x_j); c: (B, M) -> (B, n) in f64"""
    c = np.asarray(c, np.complex128)
    if len(x) == 0:
        return np.zeros((c.shape[0], n), np.complex128)
    return c @ phases(x, mode_indices(n, order), sign)


def direct_points(x, f, sign, order=0):
    """type 2: c[b, j] = sum_k f[b, k] exp(i sign k x_j); f: (B, n) -> (B, M) in f64"""
    f = np.asarray(f, np.complex128)
    if len(x) == 0:
        return np.zeros((f.shape[0], 0), np.complex128)
    return f @ phases(x, mode_indices(f.shape[1], order), sign).T


def gauss_legendre(q):
    """nodes and weights of the q-point rule on [-1, 1] in long double: Newton's iteration on P_q from the Chebyshev guess"""
    R = np.longdouble
    pi = np.arccos(R(-1))
    x = np.cos(pi * (np.arange(q, dtype=R) + R(0.75)) / (R(q) + R(0.5)))

    def legendre(x):
        p0, p1 = np.ones_like(x), x
        for j in range(2, q + 1):
            p0, p1 = p1, ((2 * j - 1) * x * p1 - (j - 1) * p0) / j
        return p1, q * (x * p1 - p0) / (x * x - 1)

    for _ in range(100):
        p, dp = legendre(x)
        x = x - p / dp
        if np.max(np.abs(p / dp)) < 1e-19:
            break
    p, dp = legendre(x)
    return x, 2 / ((1 - x * x) * dp * dp)


def phihat(w, length, kmag, nodes=None):
    """the integral over |t| <= w/2 of phi(2 t / w) cos(2 pi k t / length) for every |k| in kmag, by Gauss-Legendre in theta,
    t = (w/2) sin(theta): the integrand is entire there.  nodes=None: the handle's rule, 32 + floor(beta + pi w / 4).  In long
    double, as the handle's host code does it; returned as f64."""
    R = np.longdouble
    pi = np.arccos(R(-1))
    beta = R(2.30) * w
    q = 32 + int(2.30 * w + math.pi * w / 4) if nodes is None else nodes
    xs, ws = gauss_legendre(q)
    theta = pi / 4 * (xs + 1)
    g = pi / 4 * ws * np.exp(beta * (np.cos(theta) - 1)) * np.cos(theta) * w
    a = pi * np.asarray(kmag, R) * w / length
    return (np.cos(np.outer(a, np.sin(theta))) @ g).astype(np.float64)


class Model:
    """the handle's algorithm in numpy for n modes, accuracy eps and points x; real = the handle's precision (it sets the clamp of w),
    arith = "f64" or the handle's precision: the type the weights, the grid, the transform and the factors are held in"""

    def __init__(self, n, eps, x, real, arith="f64"):
        self.n, self.real, self.arith = n, real, arith
        self.w = w = width(eps, real)
        self.L = L = grid_length(n, w)
        T = rdt(arith)
        x = np.asarray(x, np.float64)
        xf = x - 2 * np.pi * np.floor(x / (2 * np.pi))
        xg = xf * (L / (2 * np.pi))
        xg = np.where(xg >= L, xg - L, xg)
        self.perm = np.argsort(xg, kind="stable")
        xs = xg[self.perm]
        c = np.ceil(xs - w / 2)
        self.i0 = c.astype(np.int64)
        d = (c - xs).astype(T)
        beta, ihw = T(2.30 * w), T(2) / T(w)
        t = np.arange(w).astype(T)
        z = (d[:, None] + t[None, :]) * ihw
        q = T(1) - z * z
        self.wt = np.exp(beta * (np.sqrt(np.maximum(q, T(0))) - T(1))).astype(T)  # [p, t]
        self.cells = (self.i0[:, None] + np.arange(w)[None, :]) % L
        self.inv = (1.0 / phihat(w, L, np.arange(n // 2 + 1))).astype(T)
        k = mode_indices(n, 0)
        self.cell_of_k = np.where(k < 0, k + L, k)
        self.inv_of_k = self.inv[np.abs(k)]

    def _fft(self, g, sign):
        return scipy.fft.fft(g, axis=-1) if sign < 0 else scipy.fft.ifft(g, axis=-1, norm="forward")

    def to_modes(self, c, sign, order=0):
        C = cdt(self.arith)
        c = np.asarray(c).astype(C)
        g = np.zeros((c.shape[0], self.L), C)
        if len(self.perm):
            cs = c[:, self.perm]
            for t in range(self.w):
                np.add.at(g, (slice(None), self.cells[:, t]), self.wt[None, :, t] * cs)
        f = (self._fft(g, sign).astype(C)[:, self.cell_of_k] * self.inv_of_k[None, :]).astype(C)
        return f if order == 0 else np.fft.ifftshift(f, axes=-1)

    def to_points(self, f, sign, order=0):
        C = cdt(self.arith)
        f = np.asarray(f).astype(C)
        if order == 1:
            f = np.fft.fftshift(f, axes=-1)
        g = np.zeros((f.shape[0], self.L), C)
        g[:, self.cell_of_k] = f * self.inv_of_k[None, :]
        g = self._fft(g, sign).astype(C)
        out = np.zeros((f.shape[0], len(self.perm)), C)
        if len(self.perm):
            acc = np.zeros((f.shape[0], len(self.perm)), C)
            for t in range(self.w):
                acc = (acc + self.wt[None, :, t] * g[:, self.cells[:, t]]).astype(C)
            out[:, self.perm] = acc
        return out
