"""The truth of the polyphase synthesis bank tests (tests/test_ipfb_emu.py, tests/test_gpu_ipfb.py): f64 numpy on the rounded input.

    full(frames) = (frames - 1) D + P T
    v[f, n] = 1/P sum_k Y[f, k] exp(+2 pi i k n / P)            (real rows: numpy's irfft(Y, n = P))
    y[t]    = sum over the frames f with 0 <= t - f D < P T of g[t - f D] v[f, (t - f D) mod P],   t < length

synth() inverse-transforms every frame and overlap-adds; synth_direct() is the independent statement the module checks it against when
run as a program (and tests/test_ipfb_emu.py once): the double sum over k and f written out with explicit complex exponentials and, for
real rows, the Hermitian extension of the half spectrum.  The two agree to 3e-15 relative L2 on the shapes of self_check().
ola_in_precision() is the restatement the tolerance is measured with."""
import numpy as np


def full(frames, P, T, D):
    return (frames - 1) * D + P * T


def cover(P, T, D):
    return -(-P * T // D)


def frames_in_time(Y, P, real_output):
    """(batch, frames, bins) -> (batch, frames, P) float64 / complex128: the inverse DFT of every frame"""
    Y = np.asarray(Y).astype(np.complex128)
    return np.fft.irfft(Y, n=P, axis=-1) if real_output else np.fft.ifft(Y, axis=-1)


def synth(Y, g, P, T, D, real_output, length=None):
    """Y: (batch, frames, bins) rounded input, g: P T reals (None: ones) -> (batch, length) float64 / complex128"""
    g = np.ones(P * T) if g is None else np.asarray(g, np.float64).reshape(P * T)
    v = frames_in_time(Y, P, real_output)
    batch, nf = v.shape[:2]
    w = np.tile(v, (1, 1, T)) * g  # frame f's P T weighted values: g[m] v[f, m mod P]
    y = np.zeros((batch, full(nf, P, T, D)), v.dtype)
    for f in range(nf):
        y[:, f * D: f * D + P * T] += w[:, f]
    return y[:, : y.shape[1] if length is None else length]


def synth_direct(Y, g, P, T, D, real_output, length=None):
    """The double sum, sample by sample: no FFT, no tiling.  Real rows: bins above P / 2 are the conjugates of their mirrors, and the
    imaginary parts of bin 0 and (even P) bin P / 2 are ignored, which is what makes the sum real."""
    Y = np.asarray(Y).astype(np.complex128)
    g = np.ones(P * T) if g is None else np.asarray(g, np.float64).reshape(P * T)
    batch, nf = Y.shape[:2]
    if real_output:
        spec = np.zeros((batch, nf, P), np.complex128)
        for k in range(P):
            spec[:, :, k] = Y[:, :, k] if 2 * k <= P else np.conj(Y[:, :, P - k])
        spec[:, :, 0] = spec[:, :, 0].real
        if P % 2 == 0:
            spec[:, :, P // 2] = spec[:, :, P // 2].real
    else:
        spec = Y
    n_out = full(nf, P, T, D) if length is None else length
    y = np.zeros((batch, n_out), np.complex128)
    k = np.arange(P)
    for t in range(n_out):
        for f in range(nf):
            m = t - f * D
            if 0 <= m < P * T:
                y[:, t] += g[m] / P * (spec[:, f, :] * np.exp(2j * np.pi * k * (m % P) / P)).sum(axis=-1)
    return y.real if real_output else y


def ola_in_precision(Y, g, P, T, D, real_output, length=None):
    """An exact (f64) inverse DFT rounded to the input's precision, then the filter multiply and the frame sum in that precision, in
    ascending f.  Its distance from synth() is the rounding the overlap sum adds."""
    Y = np.asarray(Y)
    rdt = Y.real.dtype
    v = frames_in_time(Y, P, real_output).astype(rdt if real_output else Y.dtype)
    g = np.ones(P * T, rdt) if g is None else np.asarray(g, rdt).reshape(P * T)
    batch, nf = v.shape[:2]
    w = np.tile(v, (1, 1, T)) * g
    assert w.dtype == v.dtype
    y = np.zeros((batch, full(nf, P, T, D)), v.dtype)
    for f in range(nf):
        y[:, f * D: f * D + P * T] += w[:, f]
    return y[:, : y.shape[1] if length is None else length]


def inverse_walk(P, T, D, frames, batch, length, fit):
    """IpfbPlan::inverse's chunks under a scratch of `fit` frames, restated from frame_plan_common.h: (b0, nb, t0, span, f_lo, nfr) per
    chunk -- whole rows where a row's frames fit, else ranges of output samples of one row from the frames that cover them, never
    fewer than cover() frames in the scratch."""
    span_pt = P * T
    if fit >= frames:
        rows_per, nfr = min(batch, fit // frames), frames
    else:
        rows_per, nfr = 1, min(frames, max(fit, cover(P, T, D)))
    if nfr == frames:
        return [(b0, min(rows_per, batch - b0), 0, length, 0, frames) for b0 in range(0, batch, rows_per)]
    chunks = []
    for b in range(batch):
        t0 = 0
        while t0 < length:
            f_lo = min((t0 - span_pt) // D + 1 if t0 >= span_pt else 0, frames - 1)
            n = min(nfr, frames - f_lo)
            t1 = length if f_lo + n >= frames else min(length, (f_lo + n) * D)
            chunks.append((b, 1, t0, t1 - t0, f_lo, n))
            t0 = t1
    return chunks


def self_check():
    rng = np.random.default_rng(0)
    worst = 0.0
    for P, T, D, real_output in ((16, 3, 5, True), (16, 4, 16, False), (9, 2, 4, True), (12, 2, 30, False), (8, 1, 4, True)):
        nf, bins = 4, (P // 2 + 1 if real_output else P)
        Y = rng.standard_normal((2, nf, bins)) + 1j * rng.standard_normal((2, nf, bins))
        g = 0.5 + rng.random(P * T)
        for length in (None, full(nf, P, T, D) - 3):
            a, b = synth(Y, g, P, T, D, real_output, length), synth_direct(Y, g, P, T, D, real_output, length)
            worst = max(worst, float(np.linalg.norm(a - b) / np.linalg.norm(a)))
    return worst


if __name__ == "__main__":
    print(self_check())
