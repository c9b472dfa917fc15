"""The cross-spectrum handle (fourier_hip_csd_*, fourier_amd.CrossSpectrum) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/csd_truth.py (f64 numpy on the
rounded input).  The `-m gpu` twin is tests/test_gpu_csd.py; this file runs its cases at the smaller sizes, both routes through
"fusion", plus the identities, the argument contract, the chunk and group walks, reserve and the bit-equal repetition.

Inputs of every accuracy check: csd_truth.pair() -- x white Gaussian, y = 0.6 roll(x, 5) + 0.8 independent noise -- and a window
0.5 + rand.  Tolerances, relative L2 over the whole output, with `base` the forward tolerance tests/test_gpu_stft.py grants the same
inner plan and precision (2e-6 f32, 1e-13 f64, doubled on a Bluestein inner plan):
  CSD        4 x base.  d(conj X Y) <= |dX||Y| + |X||dY| is 2 x the STFT's relative error against |X||Y|; over the 0.6 above, 3.3 x.
  coherence  12 x base.  Twice the CSD's error plus the two power errors of 2 x base each: 10.7 x.
Every figure is printed before it is asserted; the worst of a run, as a fraction of its bound, is printed at the end."""
import ctypes

import numpy as np
import pytest

import chunk_walks
import csd_truth as truth
import spectrogram_truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, what, route) -> the largest err / bound seen
PAIRS = {128: 16, 256: 32, 512: 16, 1024: 8, 2048: 4}  # frame pairs per workgroup of the fused kernel at f32; half as many at f64


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev
    for key, v in sorted(WORST.items()):
        print(f"csd emu worst err / bound {key}: {v:.3g}")


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (2e-13 if blu else 1e-13)


def tol(plan, real):
    return 4 * base(plan, real)


def tol_coherence(plan, real):
    return 12 * base(plan, real)


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.CrossSpectrum(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode)


def has_fused(real, n_fft):
    return n_fft in (128, 256, 512, 1024) or (n_fft == 2048 and real == "f32")


def pairs(real, n_fft):
    return PAIRS[n_fft] // (1 if real == "f32" else 2)


def csd(plan, x, y, fold=True, scale=1.0):
    """csd_ptr into a buffer that starts on an odd complex element with sentinels on both sides; checks them and that the inputs are unmodified"""
    batch, length = x.shape
    bx, by = x.tobytes(), y.tobytes()
    count = batch * plan.bins()
    buf = np.full(count + 3, SENTINEL, cdt(plan.real))
    out = buf[1:1 + count]
    plan.csd_ptr(x.ctypes.data, y.ctypes.data, out.ctypes.data, length, batch, fold, scale)
    assert buf[0] == SENTINEL and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
    assert x.tobytes() == bx and y.tobytes() == by, "csd modified an input"
    return out.reshape(batch, plan.bins()).copy()


def coherence(plan, x, y):
    batch, length = x.shape
    count = batch * plan.bins()
    buf = np.full(count + 3, SENTINEL, rdt(plan.real))
    out = buf[1:1 + count]
    plan.coherence_ptr(x.ctypes.data, y.ctypes.data, out.ctypes.data, length, batch)
    assert buf[0] == SENTINEL and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
    return out.reshape(batch, plan.bins()).copy()


def window_of(rng, real, win_length):
    return np.ascontiguousarray((0.5 + rng.random(win_length)).astype(rdt(real)))


def note(real, what, route, err, bound):
    print(f"{what} {real} {route}: err {err:.3g} bound {bound:.3g}")
    WORST[(real, what, route)] = max(WORST.get((real, what, route), 0.0), err / bound)
    assert err <= bound, (real, what, route, err, bound)


def check(fa, real, n_fft, hop, length, batch=3, pad_mode="reflect", win_length=None, seed=0):
    """both "fusion" values, the describe string asserted: CSD with the fold and scale 0.37 and the coherence against the truth, the
    two routes within tolerance of each other"""
    rng = np.random.default_rng(seed + n_fft + hop)
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    wl = plan.win_length()
    w = window_of(rng, real, wl)
    plan.set_window_ptr(w.ctypes.data)
    x, y = truth.pair(rng, batch, length, rdt(real))
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) > 0
    want_p = truth.csd(x, y, n_fft, hop, wl, w, pad_mode, True, 0.37)
    want_c = truth.coherence(x, y, n_fft, hop, wl, w, pad_mode)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        route = "fused rows" if fusion and has_fused(real, n_fft) else "composed"
        assert d.startswith(f"csd {route}, coherence {route}: real "), d
        got[fusion] = csd(plan, x, y, True, 0.37), coherence(plan, x, y)
        note(real, "csd", route, rel_l2(got[fusion][0], want_p), tol(plan, real))
        note(real, "coherence", route, rel_l2(got[fusion][1], want_c), tol_coherence(plan, real))
    assert rel_l2(got[1][0], got[0][0]) <= tol(plan, real)
    assert rel_l2(got[1][1], got[0][1]) <= tol_coherence(plan, real)
    return plan


def length_for(frames, n_fft, hop, pad_mode, extra):
    """a row length that gives `frames` frames, `extra` samples beyond the last frame's start rule"""
    return (frames - 1) * hop + extra + (n_fft if pad_mode == "none" else 0)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(fa, real):
    """frames per row = pairs per tile + 3: a row's last tile is partly empty and has pairs past the end"""
    for n in (128, 256, 2048 if real == "f32" else 1024):
        fr = pairs(real, n) + 3
        plan = check(fa, real, n, n // 4, length_for(fr, n, n // 4, "reflect", 2))                    # hop n / 4, an even length: pairs of reals
        assert plan.frames(length_for(fr, n, n // 4, "reflect", 2)) == fr
        odd = length_for(fr, n, n // 8 + 1, "reflect", 3)
        check(fa, real, n, n // 8 + 1, odd + (odd % 2 == 0))                                         # an odd hop, an odd length: single reals
        check(fa, real, n, n // 4, length_for(fr, n, n // 4, "constant", 5), pad_mode="constant")    # zero padding
        check(fa, real, n, n // 4, length_for(fr, n, n // 4, "none", 6), pad_mode="none")            # no padding: every frame interior
        check(fa, real, n, n // 4, length_for(fr, n, n // 4, "reflect", 2), win_length=n - 56)        # a shorter window


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, real):
    for n, hop, pad_mode in ((400, 100, "reflect"), (400, 37, "none"), (255, 63, "reflect"), (255, 64, "constant")):
        plan = check(fa, real, n, hop, length_for(35, n, hop, pad_mode, 3), pad_mode=pad_mode)  # 35 frames: two slots of 32, the last partly used
        plan.set_option("fusion", 1)
        assert plan.describe().startswith("csd composed, coherence composed"), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_identities(fa, real):
    rng = np.random.default_rng(17)
    for n, hop in ((256, 64), (400, 100)):
        plan = make(fa, real, n, hop)
        spec = fa.Spectrogram(n, real, hop)
        w = window_of(rng, real, n)
        plan.set_window_ptr(w.ctypes.data)
        spec.set_window_ptr(w.ctypes.data)
        x, y = truth.pair(rng, 3, 19 * hop + 2, rdt(real))
        pxx = np.empty((3, plan.bins()), rdt(real))
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            spec.set_option("fusion", fusion)
            spec.welch_ptr(x.ctypes.data, pxx.ctypes.data, x.shape[1], 3, True, 0.37)
            sxx = csd(plan, x, x, True, 0.37)
            assert rel_l2(sxx.real, pxx) <= tol(plan, real), (real, n, fusion)
            assert np.all(np.abs(sxx.imag) <= tol(plan, real) * sxx.real), (real, n, fusion)
            err = np.max(np.abs(coherence(plan, x, x) - 1))
            print(f"coherence(x, x) {real} n_fft={n} fusion={fusion}: max |C - 1| {err:.3g}")
            assert err <= tol_coherence(plan, real), (real, n, fusion)
            assert np.max(coherence(plan, x, y)) <= 1 + tol_coherence(plan, real)
            assert rel_l2(csd(plan, y, x, True, 0.37), np.conj(csd(plan, x, y, True, 0.37))) <= tol(plan, real)
            # one buffer for both signals: what x and a copy of it give, bit for bit
            x2 = x.copy()
            assert np.array_equal(csd(plan, x, x), csd(plan, x, x2)) and np.array_equal(coherence(plan, x, x), coherence(plan, x, x2))


def test_fold_and_scale(fa):
    """Bin 0, and at even n_fft the last bin, have no mirror and are never doubled; at odd n_fft every bin but 0 is."""
    rng = np.random.default_rng(2)
    for n in (16, 15):
        plan = make(fa, "f64", n, n, None, "none")
        x, y = truth.pair(rng, 1, 4 * n, np.float64)
        a, b = csd(plan, x, y, True, 2.0), csd(plan, x, y, False, 1.0)
        assert np.allclose(a, 2.0 * b * spectrogram_truth.fold_factors(n), rtol=1e-15, atol=0)


def test_chunk_and_group_walks_equal_the_unchunked_result(fa, monkeypatch):
    rng = np.random.default_rng(21)
    n, hop, length, batch = 64, 16, 300, 3   # 19 frames a row, 57 in all
    x, y = truth.pair(rng, batch, length, np.float64)
    w = truth.hann(n)
    ref = make(fa, "f64", n, hop)
    ref.set_window_ptr(w.ctypes.data)
    ref.set_option("fusion", 0)
    P, C = csd(ref, x, y, True, 2.0), coherence(ref, x, y)
    want_p, want_c = truth.csd(x, y, n, hop, n, w, "reflect", True, 2.0), truth.coherence(x, y, n, hop, n, w, "reflect")
    per_pair = 2 * ((n // 2 + 1) * 16 + n * 8)
    one_row_of_partials = 4 * (n // 2 + 1) * 8
    # 1, 2 and 3 frame pairs in the scratch; 7 and 20: chunks that end inside a row; "8" and less than a row of partials: one pair per
    # chunk and the rows walked one by one
    for bound in [k * per_pair for k in (1, 2, 3, 7, 20)] + [8, one_row_of_partials - 8]:
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(bound))
        small = make(fa, "f64", n, hop)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_window_ptr(w.ctypes.data)
        small.set_option("fusion", 0)
        # the partials of a row span several chunks: another order of the sum over frames than the unchunked walk, so within rounding
        gp, gc = csd(small, x, y, True, 2.0), coherence(small, x, y)
        assert rel_l2(gp, P) <= 1e-14 and rel_l2(gc, C) <= 1e-14, bound
        assert np.array_equal(csd(small, x, y, True, 2.0), gp), bound
        assert rel_l2(gp, want_p) <= tol(small, "f64") and rel_l2(gc, want_c) <= tol_coherence(small, "f64"), bound
    # the fused route under a bound of less than one row of partials: groups of one row, the same bits
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", "8")
    one = make(fa, "f64", 256, 64)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    big = make(fa, "f64", 256, 64)
    for plan in (one, big):
        plan.set_option("fusion", 1)
    assert one.describe().startswith("csd fused rows")
    xx, yy = truth.pair(rng, 3, 1500, np.float64)
    assert np.array_equal(csd(one, xx, yy), csd(big, xx, yy)) and np.array_equal(coherence(one, xx, yy), coherence(big, xx, yy))
    one.set_option("fusion", 0)  # and one frame pair per chunk on the composed route
    assert rel_l2(csd(one, xx, yy), truth.csd(xx, yy, 256, 64, pad_mode="reflect")) <= tol(one, "f64")


@pytest.mark.parametrize("n_fft", chunk_walks.N_FFTS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walks_at_two_slots_a_row(fa, monkeypatch, real, n_fft):
    """tests/chunk_walks.py's cases, the ones tests/test_gpu_chunks.py runs on the MI355X: 64 frames a row under bounds of 32, 64 and 96
    frame pairs (every chunk ends on a slot boundary: bit-equal to the unbounded handle) and 35 frames a row under bounds of 1 ... 40
    pairs (chunks that end inside a slot: the re-associated sums within 32 eps of the norm of sqrt(Pxx Pyy))."""
    chunk_walks.csd_chunks(chunk_walks.HostApi(fa, monkeypatch), real, n_fft)
    chunk_walks.print_worst()


@pytest.mark.parametrize("n_fft,fused", [(64, False), (250, False), (63, False), (256, True)])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_row_groups(fa, monkeypatch, real, n_fft, fused):
    """A batch of five in groups of one row and of 2, 2 and 1 rows through one partials buffer (tests/chunk_walks.py)."""
    chunk_walks.csd_groups(chunk_walks.HostApi(fa, monkeypatch), real, n_fft, fused)
    chunk_walks.print_worst()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_repetition_is_bit_equal(fa, real):
    rng = np.random.default_rng(3)
    n, hop = 256, 64
    x, y = truth.pair(rng, 3, 40 * hop + 5, rdt(real))
    plan = make(fa, real, n, hop)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        first = csd(plan, x, y), coherence(plan, x, y)
        for _ in range(9):
            again = csd(plan, x, y), coherence(plan, x, y)
            assert all(np.array_equal(a, b) for a, b in zip(first, again)), (real, fusion)


def test_truth_is_scipys(fa):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(4)
    x, y = truth.pair(rng, 3, 5000, np.float64)
    for nperseg, noverlap, scaling, onesided in ((256, None, "density", True), (255, 100, "spectrum", True), (256, 64, "density", False),
                                                 (100, 0, "spectrum", False)):
        w = truth.hann(nperseg)
        nov = nperseg // 2 if noverlap is None else noverlap
        f, want = signal.csd(x, y, fs=48.0, window=w, nperseg=nperseg, noverlap=nov, detrend=False, scaling=scaling, average="mean",
                             return_onesided=onesided)
        got = truth.csd(x, y, nperseg, nperseg - nov, nperseg, w, "none", onesided, truth.welch_scale(w, 48.0, scaling))
        if not onesided:
            want = want[:, :nperseg // 2 + 1]
        assert rel_l2(got, want) <= 1e-12, (nperseg, noverlap, scaling, onesided)
        if onesided:
            f, want = signal.coherence(x, y, fs=48.0, window=w, nperseg=nperseg, noverlap=nov, detrend=False)
            assert rel_l2(truth.coherence(x, y, nperseg, nperseg - nov, nperseg, w, "none"), want) <= 1e-12, (nperseg, noverlap)


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    for fusion in (1, 0):
        n, hop, length = 256, 64, 704
        plan = make(fa, "f64", n, hop)
        plan.set_option("fusion", fusion)
        plan.reserve(length, 3)
        x, y = truth.pair(rng, 3, length, np.float64)
        P = np.empty((3, plan.bins()), np.complex128)
        C = np.empty((3, plan.bins()))
        before = L.fourier_emu_alloc_count()
        for b in (1, 3, 2):
            plan.csd_ptr(x.ctypes.data, y.ctypes.data, P.ctypes.data, length, b)
            plan.coherence_ptr(x.ctypes.data, y.ctypes.data, C.ctypes.data, length, b)
            plan.csd_ptr(x.ctypes.data, y.ctypes.data, P.ctypes.data, length - 64, b)  # and a shorter row
        assert L.fourier_emu_alloc_count() == before, fusion


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_csd_{op}_double")  # noqa: E731
    create, run, coh, status, opt, reserve = (fn(op) for op in ("create", "csd", "coherence", "last_status", "set_option", "reserve"))
    for bad in ((0, 1, 1, 1), (8, 0, 8, 1), (8, 2, 0, 1), (8, 2, 9, 1), (8, 2, 8, 3), (8, 2, 8, -1)):
        assert not create(*bad, -1), bad
    n, hop, length = 16, 4, 40
    plan = make(fa, "f64", n, hop)
    h = plan._h
    assert (fn("n_fft")(h), fn("hop")(h), fn("win_length")(h), fn("bins")(h)) == (n, hop, n, n // 2 + 1)
    assert plan.frames(length) == 11 and fn("frames")(h, 8) == 0 and fn("frames")(h, 9) == 3  # reflect: length > p
    x, y = np.zeros((2, length)), np.ones((2, length))
    P = np.zeros((2, n // 2 + 1), np.complex128)
    C = np.zeros((2, n // 2 + 1))
    big = np.zeros(16 * x.size)
    X, Y, B = x.ctypes.data, y.ctypes.data, big.ctypes.data
    assert run(h, X, Y, P.ctypes.data, length, 2, 1, 1.0, None) == 0 and status(h) == 0
    assert run(h, None, Y, P.ctypes.data, length, 2, 1, 1.0, None) == INVALID and status(h) == INVALID
    assert run(h, X, None, P.ctypes.data, length, 2, 1, 1.0, None) == INVALID
    assert run(h, X, Y, None, length, 2, 1, 1.0, None) == INVALID
    assert run(h, X + 4, Y, P.ctypes.data, length, 1, 1, 1.0, None) == INVALID       # reals: aligned to 8 bytes
    assert run(h, X, Y + 4, P.ctypes.data, length, 1, 1, 1.0, None) == INVALID
    assert run(h, X, Y, P.ctypes.data + 8, length, 1, 1, 1.0, None) == INVALID       # complex values: aligned to 16
    assert run(h, X + 8, Y + 8, P.ctypes.data, length - 1, 1, 1, 1.0, None) == 0     # ... an odd real is enough for the inputs
    assert run(h, X, Y, P.ctypes.data, 8, 2, 1, 1.0, None) == INVALID                # an invalid length
    assert run(h, X, X, P.ctypes.data, length, 2, 1, 1.0, None) == 0                 # x and y may be one buffer
    assert run(h, B, Y, B, length, 2, 1, 1.0, None) == INVALID                       # the output on x
    assert run(h, X, B, B, length, 2, 1, 1.0, None) == INVALID                       # ... on y
    assert run(h, B, Y, B + 8 * length, length, 2, 1, 1.0, None) == INVALID          # the output begins inside x
    assert run(h, X, B, B + 8 * length, length, 2, 1, 1.0, None) == INVALID          # ... inside y
    assert run(h, X, B + 16 * 2 * (n // 2 + 1), B, length, 2, 1, 1.0, None) == 0     # y begins where the output ends: adjacent
    assert run(h, X, B + 16 * 2 * (n // 2 + 1) - 8, B, length, 2, 1, 1.0, None) == INVALID  # ... one real earlier: inside it
    assert run(h, B, Y, B + 16 * length, length, 2, 1, 1.0, None) == 0               # behind x: adjacent
    assert run(h, X, Y, P.ctypes.data, length, 0, 1, 1.0, None) == 0                 # batch 0: a no-op
    assert coh(h, X, Y, C.ctypes.data, length, 2, None) == 0 and status(h) == 0
    assert coh(h, None, Y, C.ctypes.data, length, 2, None) == INVALID and status(h) == INVALID
    assert coh(h, X, None, C.ctypes.data, length, 2, None) == INVALID
    assert coh(h, X, Y, None, length, 2, None) == INVALID
    assert coh(h, X + 4, Y, C.ctypes.data, length, 1, None) == INVALID
    assert coh(h, X, Y, C.ctypes.data + 4, length, 1, None) == INVALID
    assert coh(h, X, Y, C.ctypes.data + 8, length, 1, None) == 0                     # reals out: aligned to 8
    assert coh(h, X, Y, C.ctypes.data, 8, 2, None) == INVALID
    assert coh(h, B, Y, B, length, 2, None) == INVALID
    assert coh(h, X, B, B + 8 * length, length, 2, None) == INVALID
    assert coh(h, B, Y, B + 16 * length, length, 2, None) == 0
    assert coh(h, X, Y, C.ctypes.data, length, 0, None) == 0
    assert reserve(h, 8, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
    assert fn("set_window")(h, X + 4, None) == INVALID
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("csd composed, coherence composed")  # no fused kernel at n_fft = 16
    with pytest.raises(fa.FourierError):
        plan.csd_ptr(0, Y, P.ctypes.data, length, 1)
    with pytest.raises(fa.FourierError):
        plan.coherence_ptr(X, 0, C.ctypes.data, length, 1)
    with pytest.raises(ValueError):
        fa.CrossSpectrum(16, "f32", 4, 17)
    with pytest.raises(ValueError):
        fa.CrossSpectrum(16, "f32", 4, pad_mode="edge")
