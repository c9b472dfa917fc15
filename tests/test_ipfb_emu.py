"""The polyphase synthesis bank handle (fourier_hip_ipfb_*, fourier_amd.Ipfb) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/ipfb_truth.py (f64 numpy on the
rounded input).  The `-m gpu` twin is tests/test_gpu_ipfb.py; this file runs its cases, plus the argument contract, length(), the chunk
walk with its cuts restated, reserve, and pfb_reconstruction_terms.

Tolerance, relative L2 over the whole output: the analysis tests' figure for a transform plus one more rounding stage, twice
tests/test_gpu_real.py's tol() for the inner plan's describe string: 2 x (2e-6 f32, 1e-13 f64; Bluestein inner plans 4e-6 / 1e-11).  That
the overlap sum fits the stage: ipfb_truth.ola_in_precision (an exact inverse DFT rounded to f32, then the filter multiply and the frame
sum in f32 in ascending f) is 5e-8 ... 1e-7 from the truth for cover = 4 ... 32, a fortieth of the f32 bound
(test_the_tolerance_leaves_room_for_the_overlap_sum asserts a tenth).  A round trip through both handles gets the sum of the two
handles' tolerances."""
import ctypes

import numpy as np
import pytest

import ipfb_truth as truth
import pfb_truth
from helpers import max_rel, rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
GUARD = 64
KINDS = [("f32", False), ("f32", True), ("f64", False), ("f64", True)]


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


def bins_of(P, real_output):
    return P // 2 + 1 if real_output else P


def spectrum(rng, real, shape):
    return np.ascontiguousarray((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt(real)))


def filter_of(rng, real, P, T, prototype=False):
    """a positive-offset random filter, or the sinc-Hamming prototype"""
    import fourier_amd

    if prototype:
        return np.ascontiguousarray(fourier_amd.pfb_prototype(P, T, rdt(real)))
    return np.ascontiguousarray((0.5 + rng.random(P * T)).astype(rdt(real)))


def inverse(plan, Y, length, offset=0):
    """inverse_ptr into a buffer between guard elements (the output `offset` elements further on); checks the guards and that the input
    is unmodified"""
    batch, nf, _ = Y.shape
    by = Y.tobytes()
    buf = np.full(batch * length + 2 * GUARD + offset, SENTINEL, rdt(plan.real) if plan.real_output else cdt(plan.real))
    out = buf[GUARD + offset: GUARD + offset + batch * length]
    plan.inverse_ptr(Y.ctypes.data, out.ctypes.data, nf, length, batch)
    assert np.all(buf[: GUARD + offset] == SENTINEL) and np.all(buf[GUARD + offset + batch * length:] == SENTINEL), "a guard element was written"
    assert Y.tobytes() == by, "inverse modified its input"
    return out.reshape(batch, length).copy()


def check(fa, real, real_output, P, T, D, nf, batch, cuts=(0,), use_filter=True, prototype=False, offset=0, seed=0):
    """length = full(frames) - cut for every cut, against the truth"""
    rng = np.random.default_rng(seed + 7 * P + T + D)
    plan = fa.Ipfb(P, T, real, D, real_output)
    inner = ("real half-length: " if P % 2 == 0 else "real full-length: ") if real_output else ""
    assert plan.describe().startswith("ipfb composed: " + inner), plan.describe()
    g = filter_of(rng, real, P, T, prototype) if use_filter else None
    plan.set_filter_ptr(g.ctypes.data if use_filter else None)
    Y = spectrum(rng, real, (batch, nf, bins_of(P, real_output)))
    full = truth.full(nf, P, T, D)
    assert plan.length(nf) == full and plan.bins() == bins_of(P, real_output)
    assert (plan.channels(), plan.taps(), plan.hop()) == (P, T, D)
    for cut in cuts:
        want = truth.synth(Y, g, P, T, D, real_output, full - cut)
        got = inverse(plan, Y, full - cut, offset)
        err, emax = rel_l2(got, want), max_rel(got, want)
        assert err <= tol(plan, real), (real, real_output, P, T, D, nf, cut, err, plan.describe())
        assert emax <= 2 * tol(plan, real), (real, real_output, P, T, D, nf, cut, emax)
    return plan, Y, g, got


def sqrt_hann(P, real):
    return np.ascontiguousarray(np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(P) / P)).astype(rdt(real)))


def first_block_ones(P, T, real):
    g = np.zeros(P * T, rdt(real))
    g[:P] = 1
    return g


def test_the_truth_agrees_with_the_direct_double_sum():
    assert truth.self_check() <= 1e-13


def test_the_tolerance_leaves_room_for_the_overlap_sum():
    rng = np.random.default_rng(3)
    P = 256
    for T, D, prototype in ((4, 256, False), (3, 37, False), (16, 192, True), (8, 64, False)):  # cover 4, 21, 22, 32
        for real_output in (False, True):
            g = filter_of(rng, "f32", P, T, prototype)
            Y = spectrum(rng, "f32", (2, truth.cover(P, T, D) + 3, bins_of(P, real_output)))
            err = rel_l2(truth.ola_in_precision(Y, g, P, T, D, real_output), truth.synth(Y, g, P, T, D, real_output))
            assert err <= 4e-7, (T, D, real_output, err)


@pytest.mark.parametrize("real,real_output", KINDS)
def test_shapes(fa, real, real_output):
    P = 256
    check(fa, real, real_output, P, 4, P, 9, 3, cuts=(0, 5))                       # (a) critically sampled; a shortened, odd row
    check(fa, real, real_output, P, 3, 37, 5, 2, cuts=(0, 1))                      # (b) cover 21; odd rows: single-real stores
    check(fa, real, real_output, P, 16, 192, 30, 2, prototype=True)                # (c) oversampled prototype, cover 22
    check(fa, real, real_output, P, 4, P, 9, 3, use_filter=False)                  # (e) the default filter of ones
    check(fa, real, real_output, P, 3, 64, 6, 2, cuts=(0, 3), offset=1)            # (f) the output one element further on
    check(fa, real, real_output, 1, 3, 1, 5, 2)
    check(fa, real, real_output, 6, 2, 4, 3, 1, cuts=(0, 1))


@pytest.mark.parametrize("real,real_output", KINDS)
def test_gaps_are_exact_zeros(fa, real, real_output):
    """(d) D = P T + 8: the 8 samples between two frames are covered by none"""
    P, T = 256, 2
    D = P * T + 8
    _, _, _, y = check(fa, real, real_output, P, T, D, 3, 2)
    for f in range(2):
        gap = y[:, f * D + P * T: (f + 1) * D]
        assert gap.shape[1] == 8 and np.all(gap == 0), gap
    assert np.all(y[:, : P * T] != 0)


@pytest.mark.parametrize("real,real_output", KINDS)
def test_set_filter_null_restores_the_ones(fa, real, real_output):
    """(e)"""
    rng = np.random.default_rng(9)
    P, T, D, nf = 256, 2, 192, 4
    plan = fa.Ipfb(P, T, real, D, real_output)
    Y = spectrum(rng, real, (1, nf, plan.bins()))
    g = filter_of(rng, real, P, T)
    full = plan.length(nf)
    ones = inverse(plan, Y, full)
    plan.set_filter_ptr(g.ctypes.data)
    with_g = inverse(plan, Y, full)
    assert rel_l2(with_g, truth.synth(Y, g, P, T, D, real_output)) <= tol(plan, real)
    plan.set_filter_ptr(None)
    again = inverse(plan, Y, full)
    assert again.tobytes() == ones.tobytes() and with_g.tobytes() != ones.tobytes()
    assert rel_l2(ones, truth.synth(Y, None, P, T, D, real_output)) <= tol(plan, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_other_inner_plans(fa, real):
    """(g)"""
    for real_output in (True, False):
        for P in (400, 4096):
            plan, _, _, _ = check(fa, real, real_output, P, 2, 3 * P // 4, 3, 2, cuts=(0, 7))
            assert "stockham" in plan.describe(), plan.describe()
        for P in (255, 382):
            check(fa, real, real_output, P, 3, 3 * P // 4, 4, 2)
    plan, _, _, _ = check(fa, real, True, 63, 3, 40, 5, 2, cuts=(0, 1))
    assert plan.describe().startswith("ipfb composed: real full-length: "), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("real_rows", [True, False])
def test_round_trips_with_the_analysis_handle(fa, real, real_rows):
    """(h) the two exact pairs of include/fourier.h"""
    rng = np.random.default_rng(11)
    P, batch = 256, 2
    # T = 1, D = P / 2, h = g = the periodic sqrt-Hann window: the interior, where two frames cover every sample
    D, nf = P // 2, 7
    length = P + (nf - 1) * D
    x = rng.standard_normal((batch, length)) + (0 if real_rows else 1j * rng.standard_normal((batch, length)))
    x = np.ascontiguousarray(x.astype(rdt(real) if real_rows else cdt(real)))
    w = sqrt_hann(P, real)
    ana, syn = fa.Pfb(P, 1, real, D, real_rows), fa.Ipfb(P, 1, real, D, real_rows)
    ana.set_filter_ptr(w.ctypes.data)
    syn.set_filter_ptr(w.ctypes.data)
    X = np.empty((batch, nf, ana.bins()), cdt(real))
    ana.forward_ptr(x.ctypes.data, X.ctypes.data, length, batch)
    y = inverse(syn, X, length)
    assert rel_l2(y[:, D: nf * D], x[:, D: nf * D]) <= tol(ana, real) + tol(syn, real)
    # T = 4, D = P, h = g = ones on the first P coefficients: the first frames * P samples come back, the rest is zero
    T, nf = 4, 5
    length = P * T + (nf - 1) * P
    x = rng.standard_normal((batch, length)) + (0 if real_rows else 1j * rng.standard_normal((batch, length)))
    x = np.ascontiguousarray(x.astype(rdt(real) if real_rows else cdt(real)))
    w = first_block_ones(P, T, real)
    ana, syn = fa.Pfb(P, T, real, P, real_rows), fa.Ipfb(P, T, real, P, real_rows)
    ana.set_filter_ptr(w.ctypes.data)
    syn.set_filter_ptr(w.ctypes.data)
    assert ana.frames(length) == nf and syn.length(nf) == length
    X = np.empty((batch, nf, ana.bins()), cdt(real))
    ana.forward_ptr(x.ctypes.data, X.ctypes.data, length, batch)
    y = inverse(syn, X, length)
    assert rel_l2(y[:, : nf * P], x[:, : nf * P]) <= tol(ana, real) + tol(syn, real)
    assert np.all(y[:, nf * P:] == 0)


@pytest.mark.parametrize("real,real_output", KINDS)
def test_inverse_is_repeatable(fa, real, real_output):
    """(i)"""
    rng = np.random.default_rng(13)
    P, T, D, nf = 256, 4, 192, 12
    plan = fa.Ipfb(P, T, real, D, real_output)
    g = filter_of(rng, real, P, T, prototype=True)
    plan.set_filter_ptr(g.ctypes.data)
    Y = spectrum(rng, real, (3, nf, plan.bins()))
    first = inverse(plan, Y, plan.length(nf) - 3)
    for _ in range(3):
        assert inverse(plan, Y, plan.length(nf) - 3).tobytes() == first.tobytes()


def test_length(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    for P, T, D in ((8, 2, 8), (9, 1, 4), (4, 3, 50)):
        plan = fa.Ipfb(P, T, "f32", D, True)
        for nf in (1, 2, 7, (1 << 31) - 1):
            assert plan.length(nf) == truth.full(nf, P, T, D)
        assert plan.length(0) == 0 and plan.length(1 << 31) == 0 and plan.length((1 << 64) - 1) == 0
    big = fa.Ipfb(4, 2, "f64", (1 << 31) - 1, False)  # the largest hop and frame count: below 2^63, it fits
    assert L.fourier_hip_ipfb_length_double(big._h, (1 << 31) - 1) == ((1 << 31) - 2) * ((1 << 31) - 1) + 8


@pytest.mark.parametrize("real_output", [True, False])
def test_chunk_walks_equal_the_unbounded_result(fa, monkeypatch, real_output):
    """(k) P = 250, T = 3, D = 100 (cover 8), 20 frames, batch 3, an odd row length.  A frame takes P values of the output's kind in the
    scratch.  A bound of one frame and a bound of cover() frames both hold cover() frames: ranges inside every row; a bound of a row's
    frames plus three: whole rows, one at a time.  Real rows: the unbounded handle takes the three odd rows in one launch with single
    stores, the ranges of rows 0 and 2 start on even elements and store pairs -- the bits are the same."""
    rng = np.random.default_rng(21)
    P, T, D, nf, batch, real = 250, 3, 100, 20, 3, "f64"
    cover = truth.cover(P, T, D)
    assert cover == 8
    length = truth.full(nf, P, T, D) - 5
    Y = spectrum(rng, real, (batch, nf, bins_of(P, real_output)))
    g = filter_of(rng, real, P, T)
    ref = fa.Ipfb(P, T, real, D, real_output)
    ref.set_filter_ptr(g.ctypes.data)
    y = inverse(ref, Y, length)
    assert rel_l2(y, truth.synth(Y, g, P, T, D, real_output, length)) <= tol(ref, real)
    per = P * (8 if real_output else 16)
    for fit in (1, cover, nf + 3):
        walk = truth.inverse_walk(P, T, D, nf, batch, length, fit)
        if fit <= cover:
            assert all(c[1] == 1 and c[5] <= cover for c in walk) and walk[0] == (0, 1, 0, cover * D, 0, cover)
            assert walk[1] == (0, 1, cover * D, D, 1, cover) and len(walk) > 3 * batch  # seams inside every row
            assert sum(c[3] for c in walk) == batch * length
        else:
            assert walk == [(b, 1, 0, length, 0, nf) for b in range(batch)]
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(fit * per))
        small = fa.Ipfb(P, T, real, D, real_output)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_filter_ptr(g.ctypes.data)
        assert small.describe() == ref.describe()
        got = inverse(small, Y, length)
        assert got.tobytes() == y.tobytes(), (real_output, fit)


@pytest.mark.parametrize("real_output", [True, False])
def test_chunk_walk_over_gaps(fa, monkeypatch, real_output):
    """D = P T + 8 under a bound of two frames (cover() is 1): ranges of two frames whose last 8 samples no frame of the scratch covers,
    and which the plan must still write as zeros; bit-equal to the unbounded handle."""
    rng = np.random.default_rng(23)
    P, T, nf, batch, real = 64, 2, 7, 2, "f64"
    D = P * T + 8
    length = truth.full(nf, P, T, D) - 3
    Y = spectrum(rng, real, (batch, nf, bins_of(P, real_output)))
    g = filter_of(rng, real, P, T)
    ref = fa.Ipfb(P, T, real, D, real_output)
    ref.set_filter_ptr(g.ctypes.data)
    y = inverse(ref, Y, length)
    assert rel_l2(y, truth.synth(Y, g, P, T, D, real_output, length)) <= tol(ref, real)
    walk = truth.inverse_walk(P, T, D, nf, batch, length, 2)
    assert walk[0] == (0, 1, 0, 2 * D, 0, 2) and walk[1] == (0, 1, 2 * D, 2 * D, 2, 2) and len(walk) == 4 * batch
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(2 * P * (8 if real_output else 16)))
    small = fa.Ipfb(P, T, real, D, real_output)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    small.set_filter_ptr(g.ctypes.data)
    got = inverse(small, Y, length)
    assert got.tobytes() == y.tobytes()
    for f in range(nf - 1):
        assert np.all(got[:, f * D + P * T: (f + 1) * D] == 0)


def test_calls_after_reserve_do_not_allocate(fa, monkeypatch):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    P, T, D, nf = 256, 3, 192, 9
    for real_output in (True, False):
        for fit in (None, 5):  # whole rows; ranges of a row under a bound
            if fit is not None:
                monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(fit * P * (8 if real_output else 16)))
            plan = fa.Ipfb(P, T, "f64", D, real_output)
            if fit is not None:
                monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
            plan.reserve(nf, 3)
            Y = spectrum(rng, "f64", (3, nf, plan.bins()))
            y = np.empty((3, plan.length(nf)), np.float64 if real_output else np.complex128)
            before = L.fourier_emu_alloc_count()
            for b, frames in ((1, nf), (3, nf), (2, nf - 4)):
                plan.inverse_ptr(Y.ctypes.data, y.ctypes.data, frames, plan.length(frames), b)
            assert L.fourier_emu_alloc_count() == before, (real_output, fit)
    # What a call holds in the scratch does not grow with its frame count: under a bound of 10 frames, between one row's frames and
    # three rows', 3 rows of 7 frames go one row at a time (7 frames held) while 2 rows of 5 frames go together (10 held).  reserve()
    # covers every call of at most its frames and rows, so the call from fewer frames must not allocate either.
    P, T, D, nf, fit = 16, 2, 8, 7, 10
    for real_output in (True, False):
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(fit * P * (8 if real_output else 16)))
        plan = fa.Ipfb(P, T, "f64", D, real_output)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        assert [c[1] for c in truth.inverse_walk(P, T, D, nf, 3, plan.length(nf), fit)] == [1, 1, 1]
        assert [c[1] for c in truth.inverse_walk(P, T, D, 5, 2, plan.length(5), fit)] == [2]
        plan.reserve(nf, 3)
        Y = spectrum(rng, "f64", (3, nf, plan.bins()))
        y = np.empty((3, plan.length(nf)), np.float64 if real_output else np.complex128)
        before = L.fourier_emu_alloc_count()
        for b, frames in ((3, nf), (2, 5), (3, 3), (1, 1), (3, 6), (2, nf)):
            plan.inverse_ptr(Y.ctypes.data, y.ctypes.data, frames, plan.length(frames), b)
            assert L.fourier_emu_alloc_count() == before, (real_output, b, frames)
        want = truth.synth(Y.reshape(-1)[: 2 * 5 * plan.bins()].reshape(2, 5, plan.bins()), None, P, T, D, real_output)
        plan.inverse_ptr(Y.ctypes.data, y.ctypes.data, 5, plan.length(5), 2)
        assert rel_l2(y.reshape(-1)[: want.size].reshape(want.shape), want) <= tol(plan, "f64")


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    create, inv = L.fourier_hip_ipfb_create_double, L.fourier_hip_ipfb_inverse_double
    status, reserve = L.fourier_hip_ipfb_last_status_double, L.fourier_hip_ipfb_reserve_double
    for bad in ((0, 2, 4, 1), (8, 0, 4, 1), (8, 2, 0, 1), (8, 2, 4, 2), (8, 2, 4, -1), (1 << 16, 1 << 15, 4, 0), (8, 2, 1 << 31, 0)):
        assert not create(*bad, -1), bad
    P, T, D, nf = 16, 2, 4, 5
    for real_output in (True, False):
        plan = fa.Ipfb(P, T, "f64", D, real_output)
        h = plan._h
        bins = bins_of(P, real_output)
        assert (L.fourier_hip_ipfb_channels_double(h), L.fourier_hip_ipfb_taps_double(h), L.fourier_hip_ipfb_hop_double(h),
                L.fourier_hip_ipfb_bins_double(h)) == (P, T, D, bins)
        full = plan.length(nf)
        assert full == 48
        vs = 8 if real_output else 16  # bytes of an output value
        Y = np.zeros((2, nf, bins), np.complex128)
        y = np.zeros((2, full), np.float64 if real_output else np.complex128)
        big = np.zeros(4 * Y.size + 4 * y.size + 8, np.complex128)
        in_bytes, out_bytes = 2 * nf * bins * 16, 2 * full * vs
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, full, 2, None) == 0 and status(h) == 0
        assert inv(h, None, y.ctypes.data, nf, full, 2, None) == INVALID and status(h) == INVALID
        assert inv(h, Y.ctypes.data, None, nf, full, 2, None) == INVALID
        assert inv(h, Y.ctypes.data, y.ctypes.data, 0, full, 2, None) == INVALID            # no frames
        assert inv(h, Y.ctypes.data, y.ctypes.data, 1 << 31, full, 2, None) == INVALID      # too many
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, 0, 2, None) == INVALID              # length 0
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, full + 1, 2, None) == INVALID       # length above full(frames)
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, 1, 2, None) == 0
        assert inv(h, Y.ctypes.data + 8, y.ctypes.data, nf - 1, 1, 1, None) == INVALID      # the input: complex values, 16 bytes
        assert inv(h, Y.ctypes.data, y.ctypes.data + 4, nf, full - 1, 1, None) == INVALID   # no value is aligned to 4 bytes
        # an output a real further on: reals are aligned to sizeof(T), which is enough; complex rows aligned to sizeof(T) only are refused
        assert inv(h, Y.ctypes.data, y.ctypes.data + 8, nf, full - 1, 1, None) == (0 if real_output else INVALID)
        assert inv(h, Y.ctypes.data, y.ctypes.data + vs, nf, full - 1, 1, None) == 0
        assert inv(h, big.ctypes.data, big.ctypes.data, nf, full, 2, None) == INVALID       # in place
        assert inv(h, big.ctypes.data, big.ctypes.data + in_bytes, nf, full, 4, None) == INVALID       # the output begins inside the input
        assert inv(h, big.ctypes.data, big.ctypes.data + in_bytes, nf, full, 2, None) == 0             # adjacent
        assert inv(h, big.ctypes.data + out_bytes, big.ctypes.data, nf, full, 2, None) == 0            # ... on the other side
        assert inv(h, big.ctypes.data + out_bytes - 16, big.ctypes.data, nf, full, 2, None) == INVALID  # the input begins inside the output
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, full, 0, None) == 0 and status(h) == 0         # batch 0: a no-op
        assert inv(h, Y.ctypes.data, y.ctypes.data, nf, full + 1, 0, None) == INVALID                  # ... of valid sizes only
        assert reserve(h, 0, 1) == INVALID and reserve(h, 1 << 31, 1) == INVALID and reserve(h, nf, 0) == 0 and reserve(h, nf, 2) == 0
        assert L.fourier_hip_ipfb_set_filter_double(h, y.ctypes.data + 4, None) == INVALID
        with pytest.raises(fa.FourierError):
            plan.inverse_ptr(0, y.ctypes.data, nf, full, 1)
    with pytest.raises(ValueError):
        fa.Ipfb(16, 0)
    with pytest.raises(ValueError):
        fa.Ipfb(16, 2, hop=0)


def round_trip_terms(rng, h, g, P, T, D):
    """the coefficients of y[t] = sum_s c_s(t mod D) x[t + s P], read off a brute-force analysis -> synthesis round trip of unit
    impulses: (2 T - 1, D), from the interior samples only"""
    nf = 4 * T + 2 * truth.cover(P, T, D)
    length = truth.full(nf, P, T, D)
    lo, hi = P * T, (nf - 1) * D  # every frame that covers t exists: its start t - m >= 0 and its index <= frames - 1
    assert hi - lo >= 2 * D + 2 * P * T
    c = np.full((2 * T - 1, D), np.nan)
    x = rng.standard_normal((1, length))
    y = truth.synth(pfb_truth.pfb(x, h, P, T, D, True), g, P, T, D, True)
    for r in range(D):
        t = lo + P * T + ((r - lo - P * T) % D)  # an interior t with t mod D == r whose neighbours t + s P are interior as well
        assert t % D == r and lo <= t - (T - 1) * P and t + (T - 1) * P < hi
        for s in range(-(T - 1), T):
            e = np.zeros((1, length))
            e[0, t + s * P] = 1
            c[s + T - 1, r] = truth.synth(pfb_truth.pfb(e, h, P, T, D, True), g, P, T, D, True)[0, t]
    return c, x[0], y[0], lo, hi


def test_reconstruction_terms(fa):
    rng = np.random.default_rng(31)
    for P, T, D in ((16, 3, 5), (12, 2, 12)):
        h, g = rng.standard_normal(P * T), rng.standard_normal(P * T)
        c = fa.pfb_reconstruction_terms(h, g.reshape(T, P), P, D)
        assert c.shape == (2 * T - 1, D) and c.dtype == np.float64
        want, x, y, lo, hi = round_trip_terms(rng, h, g, P, T, D)
        assert np.abs(c - want).max() <= 1e-13 * np.abs(want).max()
        # ... and the identity itself on a random signal, over the interior
        t = np.arange(lo + P * T, hi - P * T)
        pred = sum(c[s + T - 1, t % D] * x[t + s * P] for s in range(-(T - 1), T))
        assert np.abs(pred - y[t]).max() <= 1e-13 * np.abs(y[t]).max()
    # the two exact pairs: c_0 == 1, every other term zero
    P = 32
    w = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(P) / P))
    c = fa.pfb_reconstruction_terms(w, w, P, P // 2)
    assert c.shape == (1, P // 2) and np.abs(c - 1).max() <= 4e-16
    for T in (1, 3, 4):
        w = first_block_ones(P, T, "f64")
        c = fa.pfb_reconstruction_terms(w, w, P, P)
        assert np.array_equal(c[T - 1], np.ones(P)) and np.all(np.delete(c, T - 1, axis=0) == 0)
    with pytest.raises(ValueError):
        fa.pfb_reconstruction_terms(np.ones(33), np.ones(33), 32, 16)
    with pytest.raises(ValueError):
        fa.pfb_reconstruction_terms(np.ones(64), np.ones(32), 32, 16)
