"""The MDCT handle (fourier_hip_mdct_*, fourier_amd.Mdct) WITHOUT a GPU: the engine sources compiled against the CPU emulation
(tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/mdct_truth.py (the dense cosine matrix in
f64 numpy on the rounded input).  The `-m gpu` twin is tests/test_gpu_mdct.py; this file runs its cases at the smaller sizes, every
route, both "fusion" values, plus the argument contract, the chunk walks and reserve.

Tolerance, relative L2 over the whole output: forward twice tests/test_gpu_real.py's tol() for the inner plan's describe string (a
transform plus twiddle sweeps, what tests/test_gpu_r2r.py and tests/test_gpu_stft.py grant), inverse and round trip twice that again."""
import ctypes

import numpy as np
import pytest

import mdct_truth as truth
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


def tol(plan, real, inverse=False):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return (4 if inverse else 2) * base


def prefix(n, fused):
    if n % 2:
        return "mdct full-length, imdct full-length: "
    return "mdct fused rows, imdct composed: " if fused else "mdct composed, imdct composed: "


def has_fused(real, n):
    return n in (128, 256, 512, 1024) or (n == 2048 and real == "f32")


def forward(plan, x, normalized=False):
    """forward_ptr into a buffer with a guard frame in front and behind; checks the guards and that the input is unmodified"""
    batch, length = x.shape
    nf, n = plan.frames(length), plan.size()
    bx = x.tobytes()
    buf = np.full((batch * nf + 2, n), SENTINEL, rdt(plan.real))
    plan.forward_ptr(x.ctypes.data, buf[1:].ctypes.data, length, batch, normalized)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx, "forward modified its input"
    return buf[1:-1].reshape(batch, nf, n)


def inverse(plan, X, length, normalized=False):
    batch, nf, n = X.shape
    bX = X.tobytes()
    buf = np.full((batch + 2, length), SENTINEL, rdt(plan.real))
    plan.inverse_ptr(X.ctypes.data, buf[1:].ctypes.data, nf, length, batch, normalized)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert X.tobytes() == bX, "inverse modified its input"
    return buf[1:-1]


def check_forward(fa, real, n, length, batch, center=True, window="random", normalized=False, seed=0):
    """both "fusion" values, against the truth and each other; describe() names the route"""
    rng = np.random.default_rng(seed + n + length)
    plan = fa.Mdct(n, real, center)
    w = None
    if window == "random":
        w = np.ascontiguousarray((0.5 + rng.random(2 * n)).astype(rdt(real)))
    plan.set_window_ptr(None if w is None else w.ctypes.data)
    x = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(rdt(real)))
    assert plan.frames(length) == truth.frames(length, n, center) > 0
    # the default window is the f64 sine cast to the precision
    want = truth.mdct(x, n, truth.sine_window(n, rdt(real)) if w is None else w, center, normalized)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        assert d.startswith(prefix(n, fusion == 1 and has_fused(real, n))), d
        got[fusion] = forward(plan, x, normalized)
        err = rel_l2(got[fusion], want)
        assert err <= tol(plan, real), (real, n, length, center, fusion, err, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(fa, real):
    n = 256
    check_forward(fa, real, n, 5 * n + 3, 3)                    # frames not a multiple of the tile, a workgroup spans two rows, a zero tail
    check_forward(fa, real, n, 4 * n, 2, center=False)          # no padding path
    check_forward(fa, real, n, 4 * n, 2, window=None)           # the default sine window
    check_forward(fa, real, n, 4 * n, 2, normalized=True)
    check_forward(fa, real, n, n // 2 + 1, 2)                   # a row shorter than one hop: every frame is an edge frame
    check_forward(fa, real, 128, 700, 2)
    check_forward(fa, real, 512, 1100, 1)


def test_fused_f32_1024_and_2048(fa):
    check_forward(fa, "f32", 1024, 2100, 1)
    check_forward(fa, "f32", 2048, 4100, 1)
    # f64 n = 2048: the 1024-point plan is a one-launch 32 x 32 plan, the route stays composed
    check_forward(fa, "f64", 2048, 4100, 1)


def test_input_and_output_offset_by_one_element(fa):
    rng = np.random.default_rng(5)
    for real in ("f32", "f64"):
        n, length = 256, 3 * 256 + 1
        plan = fa.Mdct(n, real)
        base = np.ascontiguousarray(rng.standard_normal(2 * length + 1).astype(rdt(real)))
        x = base[1:].reshape(2, length)
        want = truth.mdct(x, n, truth.sine_window(n, rdt(real)))
        nf = plan.frames(length)
        obase = np.empty(2 * nf * n + 1, rdt(real))
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            for off in (0, 1):  # the output on an even and on an odd element: pair stores and single stores
                out = obase[off:off + 2 * nf * n]
                out[:] = SENTINEL
                plan.forward_ptr(x.ctypes.data, out.ctypes.data, length, 2)
                assert rel_l2(out.reshape(want.shape), want) <= tol(plan, real), (real, fusion, off)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_and_full_length_shapes(fa, real):
    for n, route in ((2, "mdct composed"), (6, "mdct composed"), (160, "mdct composed"), (960, "mdct composed"), (4096, "mdct composed"),
                     (1, "mdct full-length"), (5, "mdct full-length"), (255, "mdct full-length")):
        for center in (True, False):
            plan = check_forward(fa, real, n, 5 * n + 3 if n < 4096 else 3 * n + 1, 2, center=center)
            assert plan.describe().startswith(route), plan.describe()
    check_forward(fa, real, 6, 2, 3)       # shorter than one hop
    check_forward(fa, real, 5, 10, 1, center=False, window=None)  # exactly one frame


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_inverse_matches_the_truth_and_round_trips(fa, real):
    rng = np.random.default_rng(11)
    for n in (256, 960, 255, 6, 1):
        for center in (True, False):
            plan = fa.Mdct(n, real, center)
            w = np.ascontiguousarray((0.5 + rng.random(2 * n)).astype(rdt(real)))
            plan.set_window_ptr(w.ctypes.data)
            nf = 7
            X = np.ascontiguousarray(rng.standard_normal((3, nf, n)).astype(rdt(real)))
            for length in (plan.default_length(nf), plan.default_length(nf) - n - 3 if n > 3 else plan.default_length(nf)):
                for normalized in (False, True):
                    got = inverse(plan, X, length, normalized)
                    want = truth.imdct(X, n, length, w, center, normalized)
                    assert rel_l2(got, want) <= tol(plan, real, True), (real, n, center, length, normalized)
    for n in (256, 960, 255):
        for center in (True, False):
            for window in ("sine", "pb"):
                for normalized in (False, True):
                    plan = fa.Mdct(n, real, center)
                    if window == "pb":
                        w = np.ascontiguousarray(truth.princen_bradley_window(rng, n, rdt(real)))
                        plan.set_window_ptr(w.ctypes.data)
                    length = 5 * n + 3
                    x = np.ascontiguousarray(rng.standard_normal((3, length)).astype(rdt(real)))
                    X = np.ascontiguousarray(forward(plan, x, normalized))
                    back = min(length, plan.default_length(X.shape[1]))
                    y = inverse(plan, X, back, normalized)
                    lo, hi = (0, back) if center else (n, (length // n) * n - n)  # without padding the edges carry aliasing
                    assert rel_l2(y[:, lo:hi], x[:, lo:hi]) <= tol(plan, real, True), (real, n, center, window, normalized)


def test_frames_against_the_truth(fa):
    for center in (True, False):
        for n in (1, 2, 5, 8, 16):
            plan = fa.Mdct(n, "f32", center)
            for length in range(0, 70):
                assert plan.frames(length) == truth.frames(length, n, center), (center, n, length)


def test_chunk_walks_equal_the_unchunked_result(fa, monkeypatch):
    rng = np.random.default_rng(21)
    for n in (64, 9):
        for center in (True, False):
            length, batch = 9 * n + 5, 3
            x = np.ascontiguousarray(rng.standard_normal((batch, length)))
            ref = fa.Mdct(n, "f64", center)
            ref.set_option("fusion", 0)
            X = np.ascontiguousarray(forward(ref, x))
            back = min(length, ref.default_length(X.shape[1]))
            y = inverse(ref, X, back)
            per = 2 * n * 8 if n % 2 == 0 else 4 * n * 8  # scratch bytes of one frame
            for frames_in_scratch in (1, 2, 3, 14):  # one frame forward; the inverse keeps its floor of two; 14: whole rows, one per chunk
                monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(frames_in_scratch * per))
                small = fa.Mdct(n, "f64", center)
                monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
                small.set_option("fusion", 0)
                assert np.array_equal(forward(small, x), X), (n, center, frames_in_scratch)
                assert X.shape[1] > frames_in_scratch or frames_in_scratch == 14
                assert np.array_equal(inverse(small, X, back), y), (n, center, frames_in_scratch)
            lo, hi = (0, back) if center else (n, (length // n) * n - n)
            assert rel_l2(y[:, lo:hi], x[:, lo:hi]) <= 4e-13


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    for n, fusion in ((256, 1), (256, 0), (255, 0)):
        length = 704
        plan = fa.Mdct(n, "f64")
        plan.set_option("fusion", fusion)
        plan.reserve(length, 3)
        nf = plan.frames(length)
        x = np.ascontiguousarray(rng.standard_normal((3, length)))
        X = np.empty((3, nf, n))
        y = np.empty((3, length))
        before = L.fourier_emu_alloc_count()
        for b in (1, 3, 2):
            plan.forward_ptr(x.ctypes.data, X.ctypes.data, length, b)
            plan.inverse_ptr(X.ctypes.data, y.ctypes.data, nf, length, b)
        assert L.fourier_emu_alloc_count() == before, (n, fusion)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    create, fwd, inv = L.fourier_hip_mdct_create_double, L.fourier_hip_mdct_forward_double, L.fourier_hip_mdct_inverse_double
    status, opt, reserve = L.fourier_hip_mdct_last_status_double, L.fourier_hip_mdct_set_option_double, L.fourier_hip_mdct_reserve_double
    assert not create(0, 1, -1) and not create(0, 0, -1)
    n, length = 16, 40
    for center in (True, False):
        plan = fa.Mdct(n, "f64", center)
        h = plan._h
        assert L.fourier_hip_mdct_size_double(h) == n
        nf = plan.frames(length)
        assert nf == (4 if center else 1)
        full = (nf - 1) * n if center else (nf + 1) * n
        x = np.zeros((2, max(length, full)))
        X = np.zeros((2, nf, n))
        big = np.zeros(4 * X.size + 4 * x.size)
        assert fwd(h, x.ctypes.data, X.ctypes.data, length, 2, 0, None) == 0 and status(h) == 0
        assert fwd(h, None, X.ctypes.data, length, 2, 0, None) == INVALID and status(h) == INVALID
        assert fwd(h, x.ctypes.data, None, length, 2, 0, None) == INVALID
        assert fwd(h, x.ctypes.data + 4, X.ctypes.data, length, 1, 0, None) == INVALID       # reals: aligned to 8 bytes
        assert fwd(h, x.ctypes.data, X.ctypes.data + 4, length, 1, 0, None) == INVALID
        assert fwd(h, x.ctypes.data + 8, X.ctypes.data, length - 1, 1, 0, None) == 0         # ... which is enough
        assert fwd(h, x.ctypes.data, X.ctypes.data, 0, 2, 0, None) == INVALID                # invalid lengths
        assert (fwd(h, x.ctypes.data, X.ctypes.data, 2 * n - 1, 1, 0, None) == INVALID) == (not center)
        assert fwd(h, big.ctypes.data, big.ctypes.data, length, 2, 0, None) == INVALID       # in place
        assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * length, length, 4, 0, None) == INVALID  # the output begins inside the input
        assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * 2 * length, length, 2, 0, None) == 0    # adjacent
        assert fwd(h, x.ctypes.data, X.ctypes.data, length, 0, 0, None) == 0                 # batch 0: a no-op
        assert inv(h, X.ctypes.data, x.ctypes.data, nf, full, 2, 0, None) == 0 and status(h) == 0
        assert inv(h, X.ctypes.data, x.ctypes.data, nf, 1, 2, 0, None) == 0                  # the bounds themselves are valid
        assert inv(h, X.ctypes.data, x.ctypes.data, nf, full + 1, 1, 0, None) == INVALID     # just outside either bound
        assert inv(h, X.ctypes.data, x.ctypes.data, nf, 0, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data, x.ctypes.data, 0, length, 1, 0, None) == INVALID
        assert inv(h, None, x.ctypes.data, nf, full, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data, None, nf, full, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data + 4, x.ctypes.data, nf, full, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data, x.ctypes.data + 4, nf, full, 1, 0, None) == INVALID
        assert inv(h, big.ctypes.data, big.ctypes.data, nf, full, 1, 0, None) == INVALID
        assert inv(h, X.ctypes.data, x.ctypes.data, nf, full, 0, 0, None) == 0
        assert reserve(h, 0, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
        assert L.fourier_hip_mdct_set_window_double(h, x.ctypes.data + 4, None) == INVALID
        assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
        assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("mdct composed")  # no fused kernel at n = 16: stays composed
        with pytest.raises(fa.FourierError):
            plan.forward_ptr(0, X.ctypes.data, length, 1)
    one = fa.Mdct(n, "f64", True)
    X1 = np.zeros((1, 1, n))
    assert inv(one._h, X1.ctypes.data, np.zeros(n).ctypes.data, 1, 1, 1, 0, None) == INVALID  # one centred frame gives nothing back
    with pytest.raises(ValueError):
        fa.Mdct(0, "f32")
