"""The STFT handle (fourier_hip_stft_*, fourier_amd.Stft) WITHOUT a GPU: the engine sources compiled against the CPU emulation
(tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/stft_truth.py (f64 numpy on the rounded
input).  The `-m gpu` twin is tests/test_gpu_stft.py; this file runs its cases at the smaller sizes, both routes through "fusion", plus
the argument contract, the chunk walks, reserve and the NOLA refusal.

Tolerance, relative L2 over the whole output: forward twice tests/test_gpu_real.py's tol() for the inner plan's describe string (a
transform plus one more rounding stage, the window), inverse and round trip twice that again."""
import ctypes

import numpy as np
import pytest

import stft_truth as truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def tol(plan, real, inverse=False):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return (4 if inverse else 2) * base


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.Stft(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode)


def forward(plan, x, normalized=False, offset=0):
    """forward_ptr into a buffer with a guard frame in front and behind; checks the guards and that the input is unmodified"""
    batch, length = x.shape
    nf, bins = plan.frames(length), plan.bins()
    bx = x.tobytes()
    buf = np.full((batch * nf + 2, bins), SENTINEL, cdt(plan.real))
    plan.forward_ptr(x.ctypes.data, buf[1:].ctypes.data, length, batch, normalized)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx, "forward modified its input"
    return buf[1:-1].reshape(batch, nf, bins)


def inverse(plan, X, length, normalized=False):
    batch, nf, bins = X.shape
    bX = X.tobytes()
    buf = np.full((batch + 2, length), SENTINEL, rdt(plan.real))
    plan.inverse_ptr(X.ctypes.data, buf[1:].ctypes.data, nf, length, batch, normalized)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert X.tobytes() == bX, "inverse modified its input"
    return buf[1:-1]


def window_of(rng, real, win_length):
    return np.ascontiguousarray((0.5 + rng.random(win_length)).astype(rdt(real)))


def check_forward(fa, real, n_fft, hop, length, batch, pad_mode="reflect", win_length=None, use_window=True, normalized=False, seed=0,
                  fused=True):
    """both "fusion" values where the fused route exists, against the truth and each other"""
    rng = np.random.default_rng(seed + n_fft + hop)
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    wl = plan.win_length()
    w = window_of(rng, real, wl) if use_window else None
    plan.set_window_ptr(w.ctypes.data if use_window else None)
    x = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(rdt(real)))
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) > 0
    want = truth.stft(x, n_fft, hop, wl, w, pad_mode, normalized)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        assert d.startswith("stft fused rows, istft composed: real half-length: " if fusion and fused else "stft composed, istft composed: real "), d
        got[fusion] = forward(plan, x, normalized)
        err = rel_l2(got[fusion], want)
        assert err <= tol(plan, real), (real, n_fft, hop, length, pad_mode, fusion, err, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(fa, real):
    n = 256
    check_forward(fa, real, n, n // 4, 5 * n + 3, 3)                 # frames not a multiple of the tile, a workgroup spans two rows
    check_forward(fa, real, n, 37, 2 * n + 1, 2)                     # frames start on odd elements: single reals
    check_forward(fa, real, n, n + 8, 3 * n, 2)                      # gaps between frames
    check_forward(fa, real, n, n // 4, 2 * n, 2, win_length=n - 56)  # a shorter window, even rows: pairs
    check_forward(fa, real, n, n // 4, n // 2 + 1, 2)                # both mirrors in one frame
    for pad_mode in ("none", "constant"):
        check_forward(fa, real, n, n // 2, 3 * n + 10, 2, pad_mode=pad_mode)
    check_forward(fa, real, n, n // 2, 2 * n, 1, normalized=True)
    check_forward(fa, real, n, n // 2, 2 * n, 1, use_window=False)
    check_forward(fa, real, 128, 32, 700, 2)
    check_forward(fa, real, 512, 128, 1100, 1)


def test_fused_f32_1024_and_2048(fa):
    check_forward(fa, "f32", 1024, 256, 2100, 1)
    check_forward(fa, "f32", 2048, 512, 2500, 1)
    # f64 n_fft = 2048: the 1024-point plan is a one-launch 32 x 32 plan, the route stays composed
    check_forward(fa, "f64", 2048, 512, 2500, 1, fused=False)


def test_input_offset_by_one_element(fa):
    rng = np.random.default_rng(5)
    for real in ("f32", "f64"):
        n, hop, length = 256, 64, 900
        plan = make(fa, real, n, hop)
        base = np.ascontiguousarray(rng.standard_normal(2 * length + 1).astype(rdt(real)))
        x = base[1:].reshape(2, length)
        want = truth.stft(x, n, hop)
        out = np.empty((2 * plan.frames(length), plan.bins()), cdt(real))
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            plan.forward_ptr(x.ctypes.data, out.ctypes.data, length, 2)
            assert rel_l2(out.reshape(want.shape), want) <= tol(plan, real), (real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, real):
    for n, hop, route in ((400, 160, "stockham"), (255, 64, "real full-length"), (382, 100, "bluestein"), (4096, 1024, "stockham")):
        plan = check_forward(fa, real, n, hop, 3 * n + 7, 2, fused=False)
        assert route in plan.describe(), plan.describe()
    check_forward(fa, real, 1, 1, 5, 2, fused=False)
    check_forward(fa, real, 6, 2, 9, 1, pad_mode="none", fused=False)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_inverse_matches_the_truth_and_round_trips(fa, real):
    rng = np.random.default_rng(11)
    for n, hop, pad_mode, nf, cut in ((256, 64, "reflect", 9, 0), (256, 128, "constant", 5, 17), (400, 160, "none", 4, 3), (255, 50, "reflect", 7, 0)):
        plan = make(fa, real, n, hop, None, pad_mode)
        w = window_of(rng, real, n)
        plan.set_window_ptr(w.ctypes.data)
        X = (rng.standard_normal((2, nf, plan.bins())) + 1j * rng.standard_normal((2, nf, plan.bins()))).astype(cdt(real))
        length = plan.default_length(nf) - cut
        for normalized in (False, True):
            got = inverse(plan, X, length, normalized)
            want = truth.istft(X, n, hop, length, None, w, pad_mode, normalized)
            assert rel_l2(got, want) <= tol(plan, real, True), (real, n, hop, pad_mode, normalized)
    for n, hop, pad_mode in ((256, 64, "reflect"), (256, 128, "constant"), (256, 128, "reflect")):
        plan = make(fa, real, n, hop, None, pad_mode)
        w = truth.hann(n, rdt(real))
        plan.set_window_ptr(w.ctypes.data)
        x = np.ascontiguousarray(rng.standard_normal((2, 1000)).astype(rdt(real)))
        X = forward(plan, x)
        length = plan.default_length(X.shape[1]) - 8  # an explicit, shorter length
        y = inverse(plan, np.ascontiguousarray(X), length)
        assert rel_l2(y, x[:, :length]) <= tol(plan, real, True), (real, n, hop, pad_mode)


def test_nola_refusal(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    n = 64
    plan = make(fa, "f64", n, n, None, "none")  # a Hann window with hop = n_fft: its zero at the frame edge is never covered
    w = truth.hann(n)
    plan.set_window_ptr(w.ctypes.data)
    X = np.zeros((1, 3, plan.bins()), np.complex128)
    y = np.zeros((1, 3 * n))
    assert L.fourier_hip_stft_inverse_double(plan._h, X.ctypes.data, y.ctypes.data, 3, 3 * n, 1, 0, None) == INVALID
    assert L.fourier_hip_stft_last_status_double(plan._h) == INVALID
    with pytest.raises(fa.FourierError):
        plan.inverse_ptr(X.ctypes.data, y.ctypes.data, 3, 3 * n, 1)
    plan.set_window_ptr(None)  # all ones: the envelope is 1 everywhere
    assert L.fourier_hip_stft_inverse_double(plan._h, X.ctypes.data, y.ctypes.data, 3, 3 * n, 1, 0, None) == 0


def test_frames_against_the_truth(fa):
    for pad_mode in ("none", "reflect", "constant"):
        for n, hop in ((8, 2), (9, 4), (16, 16), (16, 20)):
            plan = make(fa, "f32", n, hop, None, pad_mode)
            for length in range(0, 70):
                assert plan.frames(length) == truth.frames(length, n, hop, pad_mode), (pad_mode, n, hop, length)


def test_chunk_walks_equal_the_unchunked_result(fa, monkeypatch):
    rng = np.random.default_rng(21)
    n, hop, length, batch = 64, 16, 300, 3
    x = np.ascontiguousarray(rng.standard_normal((batch, length)))
    w = truth.hann(n)
    ref = make(fa, "f64", n, hop)
    ref.set_window_ptr(w.ctypes.data)
    ref.set_option("fusion", 0)
    X = np.ascontiguousarray(forward(ref, x))
    length = ref.default_length(X.shape[1])
    y = inverse(ref, X, length)
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(n * 8))  # ONE frame per chunk of the forward walk
    small = make(fa, "f64", n, hop)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    small.set_window_ptr(w.ctypes.data)
    small.set_option("fusion", 0)
    assert np.array_equal(forward(small, x), X)
    # the inverse keeps the n_fft / hop = 4 frames that cover one sample: ranges of 16 samples (the first one 32), seams inside every row
    assert np.array_equal(inverse(small, X, length), y)
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(7 * n * 8))  # seven frames: ranges of 64 samples (the first one 80), frames re-transformed at the seams
    mid = make(fa, "f64", n, hop)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    mid.set_window_ptr(w.ctypes.data)
    assert np.array_equal(inverse(mid, X, length), y)
    assert rel_l2(y, x[:, :length]) <= 4e-13


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    for fusion in (1, 0):
        n, hop, length = 256, 64, 704
        plan = make(fa, "f64", n, hop)
        w = truth.hann(n)
        plan.set_window_ptr(w.ctypes.data)
        plan.set_option("fusion", fusion)
        plan.reserve(length, 3)
        nf = plan.frames(length)
        x = np.ascontiguousarray(rng.standard_normal((3, length)))
        X = np.empty((3, nf, plan.bins()), np.complex128)
        y = np.empty((3, length))
        before = L.fourier_emu_alloc_count()
        for b in (1, 3, 2):
            plan.forward_ptr(x.ctypes.data, X.ctypes.data, length, b)
            plan.inverse_ptr(X.ctypes.data, y.ctypes.data, nf, length, b)
        assert L.fourier_emu_alloc_count() == before, fusion


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    create, fwd, inv = L.fourier_hip_stft_create_double, L.fourier_hip_stft_forward_double, L.fourier_hip_stft_inverse_double
    status, opt, reserve = L.fourier_hip_stft_last_status_double, L.fourier_hip_stft_set_option_double, L.fourier_hip_stft_reserve_double
    for bad in ((0, 1, 1, 1), (8, 0, 8, 1), (8, 2, 0, 1), (8, 2, 9, 1), (8, 2, 8, 3), (8, 2, 8, -1)):
        assert not create(*bad, -1), bad
    n, hop, length = 16, 4, 40
    plan = make(fa, "f64", n, hop)
    h = plan._h
    assert (L.fourier_hip_stft_n_fft_double(h), L.fourier_hip_stft_hop_double(h), L.fourier_hip_stft_win_length_double(h),
            L.fourier_hip_stft_bins_double(h)) == (n, hop, n, n // 2 + 1)
    nf = plan.frames(length)
    assert nf == 11 and L.fourier_hip_stft_frames_double(h, 8) == 0 and L.fourier_hip_stft_frames_double(h, 9) == 3  # reflect: length > p
    x = np.zeros((2, length))
    X = np.zeros((2, nf, n // 2 + 1), np.complex128)
    big = np.zeros(4 * X.size + 4 * x.size)
    assert fwd(h, x.ctypes.data, X.ctypes.data, length, 2, 0, None) == 0 and status(h) == 0
    assert fwd(h, None, X.ctypes.data, length, 2, 0, None) == INVALID and status(h) == INVALID
    assert fwd(h, x.ctypes.data, None, length, 2, 0, None) == INVALID
    assert fwd(h, x.ctypes.data + 4, X.ctypes.data, length, 1, 0, None) == INVALID       # reals: aligned to 8 bytes
    assert fwd(h, x.ctypes.data + 8, X.ctypes.data, length - 1, 1, 0, None) == 0         # ... which is enough
    assert fwd(h, x.ctypes.data, X.ctypes.data + 8, length, 1, 0, None) == INVALID       # complex values: aligned to 16 bytes
    assert fwd(h, x.ctypes.data, X.ctypes.data, 8, 2, 0, None) == INVALID                # an invalid length
    assert fwd(h, big.ctypes.data, big.ctypes.data, length, 2, 0, None) == INVALID       # in place
    assert fwd(h, big.ctypes.data, big.ctypes.data + 16 * length, length, 4, 0, None) == INVALID  # the output begins inside the input
    assert fwd(h, big.ctypes.data, big.ctypes.data + 16 * length, length, 2, 0, None) == 0        # adjacent
    assert fwd(h, x.ctypes.data, X.ctypes.data, length, 0, 0, None) == 0                 # batch 0: a no-op
    assert inv(h, X.ctypes.data, x.ctypes.data, nf, length, 2, 0, None) == 0 and status(h) == 0
    assert inv(h, X.ctypes.data, x.ctypes.data, nf, hop * (nf - 1) + 1, 1, 0, None) == INVALID  # longer than the frames give back
    assert inv(h, X.ctypes.data, x.ctypes.data, nf, 0, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data, x.ctypes.data, 0, length, 1, 0, None) == INVALID
    assert inv(h, None, x.ctypes.data, nf, length, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data, None, nf, length, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data + 8, x.ctypes.data, nf, length, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data, x.ctypes.data + 4, nf, length, 1, 0, None) == INVALID
    assert inv(h, big.ctypes.data, big.ctypes.data, nf, length, 1, 0, None) == INVALID
    assert inv(h, X.ctypes.data, x.ctypes.data, nf, length, 0, 0, None) == 0
    assert reserve(h, 8, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
    assert L.fourier_hip_stft_set_window_double(h, x.ctypes.data + 4, None) == INVALID
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("stft composed")     # no fused kernel at n_fft = 16: stays composed
    with pytest.raises(fa.FourierError):
        plan.forward_ptr(0, X.ctypes.data, length, 1)
    with pytest.raises(ValueError):
        fa.Stft(16, "f32", 4, 17)
    with pytest.raises(ValueError):
        fa.Stft(16, "f32", 4, pad_mode="edge")
