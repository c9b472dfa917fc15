"""The polyphase filter bank handle (fourier_hip_pfb_*, fourier_amd.Pfb) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/pfb_truth.py (f64 numpy on the
rounded input).  The `-m gpu` twin is tests/test_gpu_pfb.py; this file runs its cases, both routes through "fusion", plus the argument
contract, the frame count, the chunk walk and reserve.

Tolerance, relative L2 over the whole output: the STFT tests' forward tolerance, twice tests/test_gpu_real.py's tol() for the inner
plan's describe string (a transform plus one more rounding stage, here the tap sum): 2 x (2e-6 f32, 1e-13 f64; Bluestein inner plans
4e-6 / 1e-11).  That the tap sum fits the stage: pfb_truth.fold_in_precision (an f32 fold in tap order, then an exact DFT) is 4e-8 ... 8e-8
from the truth for T in {3, 4, 8, 16} with either kind of filter used here, a fiftieth of the f32 bound
(test_the_tolerance_leaves_room_for_the_tap_sum asserts a tenth)."""
import ctypes

import numpy as np
import pytest

import pfb_truth as truth
import stft_truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
COLS = 64    # no tile of the fused kernels holds more frames


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


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    return 2 * ((4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13))


def signal(rng, real, real_input, shape):
    x = rng.standard_normal(shape)
    if not real_input:
        x = x + 1j * rng.standard_normal(shape)
    return np.ascontiguousarray(x.astype(rdt(real) if real_input else cdt(real)))


def filter_of(rng, real, P, T, prototype=False):
    """a positive-offset random filter, or the sinc-Hamming prototype"""
    import fourier_amd

    if prototype:
        return np.ascontiguousarray(fourier_amd.pfb_prototype(P, T, rdt(real)))
    return np.ascontiguousarray((0.5 + rng.random(P * T)).astype(rdt(real)))


def forward(plan, x):
    """forward_ptr into a buffer with a guard frame in front and behind; checks the guards and that the input is unmodified"""
    batch, length = x.shape
    nf, bins = plan.frames(length), plan.bins()
    bx = x.tobytes()
    buf = np.full((batch * nf + 2, bins), SENTINEL, cdt(plan.real))
    plan.forward_ptr(x.ctypes.data, buf[1:].ctypes.data, length, batch)
    assert np.all(buf[0] == SENTINEL) and np.all(buf[-1] == SENTINEL), "a guard row was written"
    assert x.tobytes() == bx, "forward modified its input"
    return buf[1:-1].reshape(batch, nf, bins)


def check(fa, real, real_input, P, T, D, length, batch, fused=True, use_filter=True, prototype=False, seed=0):
    """both "fusion" values where the fused route exists, against the truth and each other"""
    rng = np.random.default_rng(seed + 7 * P + T + D)
    plan = fa.Pfb(P, T, real, D, real_input)
    h = filter_of(rng, real, P, T, prototype) if use_filter else None
    plan.set_filter_ptr(h.ctypes.data if use_filter else None)
    x = signal(rng, real, real_input, (batch, length))
    assert plan.frames(length) == truth.frames(length, P, T, D) > 0
    assert plan.bins() == (P // 2 + 1 if real_input else P)
    want = truth.pfb(x, h, P, T, D, real_input)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        inner = ("real half-length: " if P % 2 == 0 else "real full-length: ") if real_input else ""
        assert d.startswith(("pfb fused rows: " if fusion and fused else "pfb composed: ") + inner), d
        got[fusion] = forward(plan, x)
        err = rel_l2(got[fusion], want)
        assert err <= tol(plan, real), (real, real_input, P, T, D, length, fusion, err, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


KINDS = [("f32", False), ("f32", True), ("f64", False), ("f64", True)]


def test_the_truth_agrees_with_the_long_dft():
    assert truth.self_check() <= 1e-15


def test_the_tolerance_leaves_room_for_the_tap_sum():
    rng = np.random.default_rng(3)
    P, D = 256, 192
    for T in (3, 4, 8, 16):
        for prototype in (False, True):
            for real_input in (False, True):
                h = filter_of(rng, "f32", P, T, prototype)
                x = signal(rng, "f32", real_input, (2, P * T + 4 * D))
                err = rel_l2(truth.fold_in_precision(x, h, P, T, D, real_input), truth.pfb(x, h, P, T, D, real_input))
                assert err <= 4e-7, (T, prototype, real_input, err)


@pytest.mark.parametrize("real,real_input", KINDS)
def test_fused_shapes(fa, real, real_input):
    P = 256
    check(fa, real, real_input, P, 4, P, P * 4 + (COLS + 2) * P + 3, 3)                   # (a) frames not a multiple of the tile, a workgroup spans two rows
    check(fa, real, real_input, P, 3, 37, P * 3 + 2 * 37 + 1, 2)                          # (b) odd T; frames on odd elements: single reals
    check(fa, real, real_input, P, 16, 3 * P // 4, P * 16 + 4 * (3 * P // 4), 2, prototype=True)  # (c) oversampled, the longest tap loop
    check(fa, real, real_input, P, 2, P + 8, P * 2 + 2 * (P + 8), 2)                      # (d) gaps between frames
    check(fa, real, real_input, P, 4, P, P * 4 + 3 * P, 2, use_filter=False)              # (f) the default filter of all ones


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_one_tap_is_the_stft_without_padding(fa, real):
    """(e) T = 1, D = P / 2, real rows: the STFT handle with pad_mode none and the filter as its window computes the same thing"""
    rng = np.random.default_rng(8)
    P, D = 256, 128
    length = P + 5 * D
    plan = check(fa, real, True, P, 1, D, length, 2)
    h = filter_of(rng, real, P, 1)
    x = signal(rng, real, True, (2, length))
    plan.set_filter_ptr(h.ctypes.data)
    stft = fa.Stft(P, real, D, None, False)
    stft.set_window_ptr(h.ctypes.data)
    ref = np.empty((2, stft.frames(length), stft.bins()), cdt(real))
    stft.forward_ptr(x.ctypes.data, ref.ctypes.data, length, 2)
    assert rel_l2(ref, stft_truth.stft(x, P, D, P, h, "none")) <= tol(plan, real)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        assert rel_l2(forward(plan, x), ref) <= tol(plan, real), (real, fusion)


@pytest.mark.parametrize("real,real_input", KINDS)
def test_set_filter_null_restores_the_ones(fa, real, real_input):
    """(f)"""
    rng = np.random.default_rng(9)
    P, T, D = 256, 2, 256
    plan = fa.Pfb(P, T, real, D, real_input)
    x = signal(rng, real, real_input, (1, P * T + 2 * D))
    h = filter_of(rng, real, P, T)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        ones = forward(plan, x).copy()
        plan.set_filter_ptr(h.ctypes.data)
        with_h = forward(plan, x).copy()
        assert rel_l2(with_h, truth.pfb(x, h, P, T, D, real_input)) <= tol(plan, real)
        plan.set_filter_ptr(None)
        assert np.array_equal(forward(plan, x), ones) and not np.array_equal(with_h, ones)
        assert rel_l2(ones, truth.pfb(x, None, P, T, D, real_input)) <= tol(plan, real)


@pytest.mark.parametrize("real,real_input", KINDS)
def test_the_other_fused_sizes(fa, real, real_input):
    """(g) one case per other fused P of the kind; f64 at the top size stays composed"""
    k = 2 if real_input else 1
    for P in (64 * k, 128 * k, 512 * k):
        check(fa, real, real_input, P, 2, P, P * 2 + COLS * P, 1)
    check(fa, real, real_input, 1024 * k, 2, 1024 * k, 1024 * k * 2 + 8 * 1024 * k, 1, fused=real == "f32")


def test_input_offset_by_one_element(fa):
    """real rows that start on an odd element: the pairs flag is off"""
    rng = np.random.default_rng(5)
    for real in ("f32", "f64"):
        P, T, D = 256, 3, 64
        length = P * T + 4 * D
        plan = fa.Pfb(P, T, real, D, True)
        h = filter_of(rng, real, P, T)
        plan.set_filter_ptr(h.ctypes.data)
        base = signal(rng, real, True, 2 * length + 1)
        x = base[1:].reshape(2, length)
        want = truth.pfb(x, h, P, T, D, True)
        out = np.empty((2 * plan.frames(length), plan.bins()), cdt(real))
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            plan.forward_ptr(x.ctypes.data, out.ctypes.data, length, 2)
            assert rel_l2(out.reshape(want.shape), want) <= tol(plan, real), (real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, real):
    routes = {(400, True): "stockham", (255, True): "real full-length", (382, True): "bluestein", (4096, True): "stockham",
              (400, False): "stockham", (255, False): "bluestein", (382, False): "bluestein", (4096, False): "stockham"}
    for real_input in (True, False):
        for P in (400, 255, 382, 4096):
            plan = check(fa, real, real_input, P, 3, 3 * P // 4, 3 * P + 2 * (3 * P // 4) + 5, 2, fused=False)
            assert routes[(P, real_input)] in plan.describe(), plan.describe()
        check(fa, real, real_input, 1, 3, 1, 7, 2, fused=False)
        check(fa, real, real_input, 6, 2, 4, 12 + 9, 1, fused=False)


def test_frames_against_the_truth(fa):
    for P, T, D in ((8, 2, 8), (9, 1, 4), (4, 3, 5), (16, 2, 20)):
        plan = fa.Pfb(P, T, "f32", D, True)
        for length in range(0, P * T + 3 * D + 1):
            assert plan.frames(length) == truth.frames(length, P, T, D), (P, T, D, length)


def test_chunk_walk_equals_the_unchunked_result(fa, monkeypatch):
    rng = np.random.default_rng(21)
    P, T, D, batch = 64, 3, 48, 3
    length = P * T + 10 * D + 5
    for real_input in (True, False):
        x = signal(rng, "f64", real_input, (batch, length))
        h = filter_of(rng, "f64", P, T)
        ref = fa.Pfb(P, T, "f64", D, real_input)
        ref.set_filter_ptr(h.ctypes.data)
        ref.set_option("fusion", 0)
        X = forward(ref, x).copy()
        assert rel_l2(X, truth.pfb(x, h, P, T, D, real_input)) <= tol(ref, "f64")
        frame_bytes = P * (8 if real_input else 16)
        for frames_in_scratch in (1, 7):
            monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(frames_in_scratch * frame_bytes))
            small = fa.Pfb(P, T, "f64", D, real_input)
            monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
            small.set_filter_ptr(h.ctypes.data)
            small.set_option("fusion", 0)
            assert small.describe().startswith("pfb composed")
            assert np.array_equal(forward(small, x), X), (real_input, frames_in_scratch)


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    for real_input in (True, False):
        for fusion in (1, 0):
            P, T, D = 256, 3, 192
            length = P * T + 6 * D
            plan = fa.Pfb(P, T, "f64", D, real_input)
            plan.set_option("fusion", fusion)
            plan.reserve(length, 3)
            x = signal(rng, "f64", real_input, (3, length))
            X = np.empty((3, plan.frames(length), plan.bins()), np.complex128)
            before = L.fourier_emu_alloc_count()
            for b in (1, 3, 2):
                plan.forward_ptr(x.ctypes.data, X.ctypes.data, length, b)
            assert L.fourier_emu_alloc_count() == before, (real_input, fusion)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    create, fwd = L.fourier_hip_pfb_create_double, L.fourier_hip_pfb_forward_double
    status, opt, reserve = L.fourier_hip_pfb_last_status_double, L.fourier_hip_pfb_set_option_double, L.fourier_hip_pfb_reserve_double
    for bad in ((0, 2, 4, 1), (8, 0, 4, 1), (8, 2, 0, 1), (8, 2, 4, 2), (8, 2, 4, -1), (1 << 16, 1 << 15, 4, 0), (8, 2, 1 << 31, 0)):
        assert not create(*bad, -1), bad
    P, T, D, length = 16, 2, 4, 48
    for real_input in (True, False):
        plan = fa.Pfb(P, T, "f64", D, real_input)
        h = plan._h
        bins = P // 2 + 1 if real_input else P
        assert (L.fourier_hip_pfb_channels_double(h), L.fourier_hip_pfb_taps_double(h), L.fourier_hip_pfb_hop_double(h),
                L.fourier_hip_pfb_bins_double(h)) == (P, T, D, bins)
        nf = plan.frames(length)
        assert nf == 5 and L.fourier_hip_pfb_frames_double(h, P * T - 1) == 0 and L.fourier_hip_pfb_frames_double(h, P * T) == 1
        vs = 8 if real_input else 16  # bytes of an input value
        x = np.zeros((2, length), np.float64 if real_input else np.complex128)
        X = np.zeros((2, nf, bins), np.complex128)
        big = np.zeros(4 * X.size + 4 * x.size + 8, np.complex128)
        assert fwd(h, x.ctypes.data, X.ctypes.data, length, 2, None) == 0 and status(h) == 0
        assert fwd(h, None, X.ctypes.data, length, 2, None) == INVALID and status(h) == INVALID
        assert fwd(h, x.ctypes.data, None, length, 2, None) == INVALID
        assert fwd(h, x.ctypes.data + 4, X.ctypes.data, length, 1, None) == INVALID         # no value is aligned to 4 bytes
        # a value further on: reals are aligned to sizeof(T), which is enough; a complex input aligned to sizeof(T) only is refused
        assert fwd(h, x.ctypes.data + 8, X.ctypes.data, length - 1, 1, None) == (0 if real_input else INVALID)
        assert fwd(h, x.ctypes.data + vs, X.ctypes.data, length - 1, 1, None) == 0
        assert fwd(h, x.ctypes.data, X.ctypes.data + 8, length, 1, None) == INVALID         # complex values: aligned to 16 bytes
        assert fwd(h, x.ctypes.data, X.ctypes.data, P * T - 1, 2, None) == INVALID          # an invalid length
        assert fwd(h, big.ctypes.data, big.ctypes.data, length, 2, None) == INVALID         # in place
        assert fwd(h, big.ctypes.data, big.ctypes.data + 2 * vs * length, length, 4, None) == INVALID  # the output begins inside the input
        assert fwd(h, big.ctypes.data, big.ctypes.data + 2 * vs * length, length, 2, None) == 0        # adjacent
        assert fwd(h, big.ctypes.data + 2 * 16 * nf * bins, big.ctypes.data, length, 2, None) == 0     # ... on the other side
        assert fwd(h, big.ctypes.data + 2 * 16 * nf * bins - 16, big.ctypes.data, length, 2, None) == INVALID  # the input begins inside the output
        assert fwd(h, x.ctypes.data, X.ctypes.data, length, 0, None) == 0                   # batch 0: a no-op
        assert reserve(h, P * T - 1, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
        assert L.fourier_hip_pfb_set_filter_double(h, x.ctypes.data + 4, None) == INVALID
        assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
        assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("pfb composed")     # no fused kernel at P = 16: stays composed
        with pytest.raises(fa.FourierError):
            plan.forward_ptr(0, X.ctypes.data, length, 1)
    with pytest.raises(ValueError):
        fa.Pfb(16, 0)
    with pytest.raises(ValueError):
        fa.Pfb(16, 2, hop=0)


def test_prototype_is_the_windowed_sinc(fa):
    P, T = 8, 4
    n = np.arange(P * T)
    want = np.sinc((n - (P * T - 1) / 2) / P) * np.hamming(P * T)
    assert np.array_equal(fa.pfb_prototype(P, T), want)
    assert np.array_equal(fa.pfb_prototype(P, T, np.float32), want.astype(np.float32))
