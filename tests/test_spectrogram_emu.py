"""The spectrogram handle (fourier_hip_spectrogram_*, fourier_amd.Spectrogram) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/spectrogram_truth.py (f64 numpy
on the rounded input).  The `-m gpu` twin is tests/test_gpu_spectrogram.py; this file runs its cases at the smaller sizes, both routes
through "fusion", plus the argument contract, the chunk walks, reserve and the bit-equal repetition.

Tolerance, relative L2 over the whole output on white Gaussian input: twice what tests/test_stft_emu.py's tol() grants the forward STFT
of the same inner plan (d|X|^2 = 2 Re(conj X dX): about 1.4 x the STFT's relative error; a square root or a mean does not raise it).
The worst figure of each run must stay below HALF the bound here, the condition for taking the kernels to the GPU."""
import ctypes

import numpy as np
import pytest

import chunk_walks
import spectrogram_truth as truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, route) -> the largest err / bound seen


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
        print(f"spectrogram emu worst err / bound {key}: {v:.3g}")


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return 2 * 2 * base  # twice the STFT's forward tolerance


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.Spectrogram(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode)


def forward(plan, x, power=2, normalized=False):
    """forward_ptr into a buffer with a guard frame in front and behind; checks the guards and that the input is unmodified"""
    batch, length = x.shape
    nf, bins = plan.frames(length), plan.bins()
    bx = x.tobytes()
    buf = np.full((batch * nf + 2, bins), SENTINEL, rdt(plan.real))
    plan.forward_ptr(x.ctypes.data, buf[1:].ctypes.data, length, batch, power, normalized)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx, "forward modified its input"
    return buf[1:-1].reshape(batch, nf, bins).copy()


def welch(plan, x, fold=True, scale=1.0):
    batch, length = x.shape
    bx = x.tobytes()
    buf = np.full((batch + 2, plan.bins()), SENTINEL, rdt(plan.real))
    plan.welch_ptr(x.ctypes.data, buf[1:].ctypes.data, length, batch, fold, scale)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx, "welch modified its input"
    return buf[1:-1].copy()


def window_of(rng, real, win_length):
    return np.ascontiguousarray((0.5 + rng.random(win_length)).astype(rdt(real)))


def note(real, route, err, bound):
    WORST[(real, route)] = max(WORST.get((real, route), 0.0), err / bound)
    assert err <= bound / 2, (real, route, err, bound)  # below half the bound on the emulator (and so below the bound)


def check(fa, real, n_fft, hop, length, batch, pad_mode="reflect", win_length=None, use_window=True, seed=0, fused=True):
    """both "fusion" values where the fused route exists: power 1 and 2, normalized on and off, Welch with and without the fold"""
    rng = np.random.default_rng(seed + n_fft + hop)
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    wl = plan.win_length()
    w = window_of(rng, real, wl) if use_window else None
    plan.set_window_ptr(w.ctypes.data if use_window else None)
    x = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(rdt(real)))
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) > 0
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        route = "fused rows" if fusion and fused else "composed"
        assert d.startswith(f"spectrogram {route}, welch {route}: real "), d
        assert "real half-length: " in d or route == "composed", d
        for power in (1, 2):
            for normalized in (False, True):
                want = truth.spectrogram(x, n_fft, hop, wl, w, pad_mode, power, normalized)
                got[fusion, power, normalized] = forward(plan, x, power, normalized)
                note(real, "spectrogram " + route, rel_l2(got[fusion, power, normalized], want), tol(plan, real))
        for fold in (True, False):
            want = truth.welch(x, n_fft, hop, wl, w, pad_mode, fold, 0.37)
            got[fusion, "welch", fold] = welch(plan, x, fold, 0.37)
            note(real, "welch " + route, rel_l2(got[fusion, "welch", fold], want), tol(plan, real))
    for key in [k[1:] for k in got if k[0] == 1]:
        assert rel_l2(got[(1,) + key], got[(0,) + key]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(fa, real):
    n = 256
    cols = 64 if real == "f32" else 32  # frames per workgroup at n_fft 256: frames = cols + 3 leaves the last tile partly empty
    check(fa, real, n, n // 4, (cols + 2) * (n // 4) + 3, 3)           # frames not a multiple of the tile, a workgroup spans two rows
    check(fa, real, n, 37, 3 * n + 1, 2)                               # frames start on odd elements, an odd length: single reals
    check(fa, real, n, n // 4, 2 * n, 2, win_length=n - 56)            # a shorter window, even rows: pairs
    check(fa, real, n, n // 4, n // 2 + 1, 2)                          # both mirrors in one frame
    for pad_mode in ("none", "constant"):
        check(fa, real, n, n // 2, 3 * n + 10, 2, pad_mode=pad_mode)
    check(fa, real, n, n // 2, 2 * n, 1, use_window=False)
    check(fa, real, 128, 32, 700, 2)
    check(fa, real, 512, 128, 1100, 1)


def test_fused_f32_1024_and_2048(fa):
    check(fa, "f32", 1024, 256, 2100, 1)
    check(fa, "f32", 2048, 512, 2500, 1)
    check(fa, "f64", 2048, 512, 2500, 1, fused=False)  # the f64 1024-point plan has no row kernel: composed


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, real):
    for n, hop, route in ((400, 160, "stockham"), (255, 64, "real full-length"), (382, 100, "bluestein")):
        for pad_mode in ("reflect", "none", "constant"):
            plan = check(fa, real, n, hop, 3 * n + 7, 2, pad_mode=pad_mode, fused=False)
            assert route in plan.describe(), plan.describe()
    check(fa, real, 1, 1, 5, 2, fused=False)
    check(fa, real, 6, 2, 9, 1, pad_mode="none", fused=False)
    check(fa, real, 64, 3, 64 + 3 * 70, 2, pad_mode="none", fused=False)  # 71 frames a row: three slots of 32 frames, the last partly used


def test_fold_factors_at_odd_and_even_n_fft(fa):
    """Bin 0, and at even n_fft the last bin, have no mirror and are never doubled; at odd n_fft every bin but 0 is."""
    for n in (16, 15):
        plan = make(fa, "f64", n, n, None, "none")
        x = np.ascontiguousarray(np.random.default_rng(n).standard_normal((1, 4 * n)))
        a, b = welch(plan, x, True), welch(plan, x, False)
        c = truth.fold_factors(n)
        assert c[0] == 1 and np.all(c[1:(n - 1) // 2 + 1] == 2) and (n % 2 == 1 or c[-1] == 1)
        assert np.allclose(a, b * c, rtol=1e-15, atol=0)


def test_chunk_walks_equal_the_unchunked_result(fa, monkeypatch):
    rng = np.random.default_rng(21)
    n, hop, length, batch = 64, 16, 300, 3   # 19 frames a row, 57 in all
    x = np.ascontiguousarray(rng.standard_normal((batch, length)))
    w = truth.hann(n)
    ref = make(fa, "f64", n, hop)
    ref.set_window_ptr(w.ctypes.data)
    ref.set_option("fusion", 0)
    P, M, W = forward(ref, x, 2), forward(ref, x, 1, True), welch(ref, x, True, 2.0)
    per_frame = (n // 2 + 1) * 16 + n * 8
    for k in (1, 2, 3, 7, 20):  # 1, 2 and 3 frames in the scratch; 7 and 20: chunks that end inside a row
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(k * per_frame))
        small = make(fa, "f64", n, hop)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_window_ptr(w.ctypes.data)
        small.set_option("fusion", 0)
        assert np.array_equal(forward(small, x, 2), P) and np.array_equal(forward(small, x, 1, True), M), k
        # the partials of a row span several chunks: another order of the sum over frames than the unchunked walk, so within rounding
        got = welch(small, x, True, 2.0)
        assert rel_l2(got, W) <= 1e-14, k
        assert np.array_equal(welch(small, x, True, 2.0), got), k
        # the bound also holds one row of partials only (33 reals): the rows are walked one by one
        assert rel_l2(got, truth.welch(x, n, hop, n, w, "reflect", True, 2.0)) <= tol(small, "f64") / 2
    # the fused Welch under a bound of one row of partials: groups of one row
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", "8")
    one = make(fa, "f64", 256, 64)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    big = make(fa, "f64", 256, 64)
    for plan in (one, big):
        plan.set_option("fusion", 1)
    assert one.describe().startswith("spectrogram fused rows")
    xx = np.ascontiguousarray(rng.standard_normal((3, 1500)))
    assert np.array_equal(welch(one, xx), welch(big, xx))
    one.set_option("fusion", 0)  # and one frame per chunk on the composed route
    assert rel_l2(welch(one, xx), truth.welch(xx, 256, 64, pad_mode="reflect")) <= tol(one, "f64") / 2


@pytest.mark.parametrize("n_fft", chunk_walks.N_FFTS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walks_at_two_slots_a_row(fa, monkeypatch, real, n_fft):
    """tests/chunk_walks.py's cases, the ones tests/test_gpu_chunks.py runs on the MI355X: 64 frames a row under bounds of 32, 64 and 96
    frames (every chunk ends on a slot boundary: bit-equal to the unbounded handle) and 35 frames a row under bounds of 1 ... 40 frames
    (chunks that end inside a slot: the re-associated sum within 32 eps of the truth's norm)."""
    chunk_walks.spectrogram_chunks(chunk_walks.HostApi(fa, monkeypatch), real, n_fft)
    chunk_walks.print_worst()


@pytest.mark.parametrize("n_fft,fused", [(64, False), (250, False), (63, False), (256, True)])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_row_groups(fa, monkeypatch, real, n_fft, fused):
    """A batch of five in groups of one row and of 2, 2 and 1 rows through one partials buffer (tests/chunk_walks.py)."""
    chunk_walks.welch_groups(chunk_walks.HostApi(fa, monkeypatch), real, n_fft, fused)
    chunk_walks.print_worst()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_repetition_is_bit_equal(fa, real):
    rng = np.random.default_rng(3)
    n, hop = 256, 64
    x = np.ascontiguousarray(rng.standard_normal((3, 11 * hop + 5)).astype(rdt(real)))
    plan = make(fa, real, n, hop)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        first = forward(plan, x, 2), forward(plan, x, 1), welch(plan, x)
        for _ in range(3):
            again = forward(plan, x, 2), forward(plan, x, 1), welch(plan, x)
            assert all(np.array_equal(a, b) for a, b in zip(first, again)), (real, fusion)


def test_welch_equals_the_mean_of_the_power_spectrogram(fa):
    rng = np.random.default_rng(8)
    for real in ("f32", "f64"):
        for n, hop in ((256, 64), (400, 160)):
            plan = make(fa, real, n, hop, None, "none")
            w = truth.hann(n, rdt(real))
            plan.set_window_ptr(w.ctypes.data)
            x = np.ascontiguousarray(rng.standard_normal((2, 9 * n + 11)).astype(rdt(real)))
            for fusion in (1, 0):
                plan.set_option("fusion", fusion)
                mean = forward(plan, x, 2).astype(np.float64).mean(axis=1)
                assert rel_l2(welch(plan, x, False, 1.0), mean) <= tol(plan, real), (real, n, fusion)


def test_truth_welch_is_scipys(fa):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 5000))
    for nperseg, noverlap, scaling, onesided in ((256, None, "density", True), (255, 100, "spectrum", True), (256, 64, "density", False),
                                                 (100, 0, "spectrum", False)):
        w = truth.hann(nperseg)
        nov = nperseg // 2 if noverlap is None else noverlap
        f, want = signal.welch(x, fs=48.0, window=w, nperseg=nperseg, noverlap=nov, detrend=False, scaling=scaling, average="mean",
                               return_onesided=onesided)
        got = truth.welch(x, nperseg, nperseg - nov, nperseg, w, "none", onesided, truth.welch_scale(w, 48.0, scaling))
        if not onesided:
            want, f = want[:, :nperseg // 2 + 1], f[:nperseg // 2 + 1]
        assert np.allclose(np.abs(f), np.arange(nperseg // 2 + 1) * 48.0 / nperseg, rtol=1e-14)  # (two-sided: scipy's Nyquist bin is -fs / 2)
        assert rel_l2(got, want) <= 1e-12, (nperseg, noverlap, scaling, onesided)


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
        nf = plan.frames(length)
        x = np.ascontiguousarray(rng.standard_normal((3, length)))
        S = np.empty((3, nf, plan.bins()))
        P = np.empty((3, plan.bins()))
        before = L.fourier_emu_alloc_count()
        for b in (1, 3, 2):
            plan.forward_ptr(x.ctypes.data, S.ctypes.data, length, b)
            plan.welch_ptr(x.ctypes.data, P.ctypes.data, length, b)
            plan.welch_ptr(x.ctypes.data, P.ctypes.data, length - 64, b)  # and a shorter row
        assert L.fourier_emu_alloc_count() == before, fusion


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_spectrogram_{op}_double")  # noqa: E731
    create, fwd, wel, status, opt, reserve = (fn(op) for op in ("create", "forward", "welch", "last_status", "set_option", "reserve"))
    for bad in ((0, 1, 1, 1), (8, 0, 8, 1), (8, 2, 0, 1), (8, 2, 9, 1), (8, 2, 8, 3), (8, 2, 8, -1)):
        assert not create(*bad, -1), bad
    n, hop, length = 16, 4, 40
    plan = make(fa, "f64", n, hop)
    h = plan._h
    assert (fn("n_fft")(h), fn("hop")(h), fn("win_length")(h), fn("bins")(h)) == (n, hop, n, n // 2 + 1)
    nf = plan.frames(length)
    assert nf == 11 and fn("frames")(h, 8) == 0 and fn("frames")(h, 9) == 3  # reflect: length > p
    x = np.zeros((2, length))
    S = np.zeros((2, nf, n // 2 + 1))
    P = np.zeros((2, n // 2 + 1))
    big = np.zeros(4 * S.size + 4 * x.size)
    assert fwd(h, x.ctypes.data, S.ctypes.data, length, 2, 2, 0, None) == 0 and status(h) == 0
    assert fwd(h, x.ctypes.data, S.ctypes.data, length, 2, 1, 1, None) == 0
    for power in (0, 3, -1):
        assert fwd(h, x.ctypes.data, S.ctypes.data, length, 2, power, 0, None) == INVALID and status(h) == INVALID
    assert fwd(h, None, S.ctypes.data, length, 2, 2, 0, None) == INVALID
    assert fwd(h, x.ctypes.data, None, length, 2, 2, 0, None) == INVALID
    assert fwd(h, x.ctypes.data + 4, S.ctypes.data, length, 1, 2, 0, None) == INVALID       # reals: aligned to 8 bytes
    assert fwd(h, x.ctypes.data, S.ctypes.data + 4, length, 1, 2, 0, None) == INVALID
    assert fwd(h, x.ctypes.data + 8, S.ctypes.data + 8, length - 1, 1, 2, 0, None) == 0     # ... which is enough, on both sides
    assert fwd(h, x.ctypes.data, S.ctypes.data, 8, 2, 2, 0, None) == INVALID                # an invalid length
    assert fwd(h, big.ctypes.data, big.ctypes.data, length, 2, 2, 0, None) == INVALID       # in place
    assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * length, length, 4, 2, 0, None) == INVALID  # the output begins inside the input
    assert fwd(h, big.ctypes.data, big.ctypes.data + 16 * length, length, 2, 2, 0, None) == 0       # adjacent
    assert fwd(h, x.ctypes.data, S.ctypes.data, length, 0, 2, 0, None) == 0                 # batch 0: a no-op
    assert wel(h, x.ctypes.data, P.ctypes.data, length, 2, 1, 1.0, None) == 0 and status(h) == 0
    assert wel(h, None, P.ctypes.data, length, 2, 1, 1.0, None) == INVALID and status(h) == INVALID
    assert wel(h, x.ctypes.data, None, length, 2, 1, 1.0, None) == INVALID
    assert wel(h, x.ctypes.data + 4, P.ctypes.data, length, 1, 1, 1.0, None) == INVALID
    assert wel(h, x.ctypes.data, P.ctypes.data + 4, length, 1, 1, 1.0, None) == INVALID
    assert wel(h, x.ctypes.data, P.ctypes.data, 8, 2, 1, 1.0, None) == INVALID
    assert wel(h, big.ctypes.data, big.ctypes.data, length, 2, 1, 1.0, None) == INVALID
    assert wel(h, big.ctypes.data, big.ctypes.data + 8 * length, length, 2, 1, 1.0, None) == INVALID
    assert wel(h, big.ctypes.data, big.ctypes.data + 16 * length, length, 2, 1, 1.0, None) == 0
    assert wel(h, x.ctypes.data, P.ctypes.data, length, 0, 1, 1.0, None) == 0
    assert reserve(h, 8, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
    assert fn("set_window")(h, x.ctypes.data + 4, None) == INVALID
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("spectrogram composed, welch composed")  # no fused kernel at n_fft = 16
    with pytest.raises(fa.FourierError):
        plan.forward_ptr(0, S.ctypes.data, length, 1)
    with pytest.raises(ValueError):
        fa.Spectrogram(16, "f32", 4, 17)
    with pytest.raises(ValueError):
        fa.Spectrogram(16, "f32", 4, pad_mode="edge")
