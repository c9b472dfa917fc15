"""The band-spectrogram handle (fourier_hip_bandspec_*, fourier_amd.BandSpectrogram) WITHOUT a GPU: the engine sources compiled against
the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/bandspec_truth.py.
The `-m gpu` twin is tests/test_gpu_bandspec.py; both run the shapes, banks, assertions, tolerances and output guards of
tests/bandspec_cases.py.  This file adds the argument contract, forward before set_bands, a NaN weight, a bad log_floor, the
allocation-free property after reserve, and the chunk walk under a small scratch bound, bit-equal to the unbounded handle."""
import ctypes

import numpy as np
import pytest

import bandspec_cases as cases
import bandspec_truth as truth

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


class HostApi:
    """device memory is host memory on the emulator"""

    def __init__(self, fa):
        self.fa = fa

    def make(self, real, n_fft, bands, hop, win_length=None, pad_mode="reflect"):
        return self.fa.BandSpectrogram(n_fft, bands, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode)

    def upload(self, a):
        return np.ascontiguousarray(a)

    def set_window(self, plan, w):
        plan.set_window_ptr(w.ctypes.data)

    def forward(self, plan, x, batch, length, power, normalized, log_mult, log_floor):
        count = batch * plan.frames(length) * plan.bands()
        bx = x.tobytes()
        buf = np.full(count + 3, SENTINEL, x.dtype)
        out = buf[1:1 + count]
        assert out.ctypes.data % (2 * x.itemsize) != 0  # the output starts on an odd element
        plan.forward_ptr(x.ctypes.data, out.ctypes.data, length, batch, power, normalized, log_mult, log_floor)
        assert buf[0] == SENTINEL and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
        assert x.tobytes() == bx, "forward modified its input"
        return out.reshape(batch, plan.frames(length), plan.bands()).copy()


@pytest.fixture(scope="module")
def api(fa):
    return HostApi(fa)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(api, real):
    cases.fused_shapes(api, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_xcds(api, real):
    cases.more_workgroups_than_xcds(api, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(api, real):
    cases.composed_only_shapes(api, real)


@pytest.mark.parametrize("kind", cases.BANK_KINDS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_banks(api, real, kind):
    cases.banks(api, real, kind)


@pytest.mark.parametrize("real,n_fft", [("f32", 128), ("f32", 512), ("f32", 1024), ("f64", 128), ("f64", 512)])
def test_the_other_fused_lengths(api, real, n_fft):
    """the instantiations the shared cases do not reach (they run 256 and the largest: 2048 at f32, 1024 at f64)"""
    cases.check(api, real, n_fft, n_fft // 4, "reflect", extra=3, batch=2)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_repetition_is_bit_equal_and_a_new_bank_replaces_the_old(api, real):
    rng = np.random.default_rng(5)
    n, hop, batch = 256, 64, 3
    length = 11 * hop + 5
    x = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(cases.np_real(real)))
    plan = api.make(real, n, 40, hop)
    W = cases.mel_bank(n)
    plan.set_bands(W)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        first = api.forward(plan, x, batch, length, 2, False, 0.0, 0.0)
        for _ in range(3):
            assert np.array_equal(api.forward(plan, x, batch, length, 2, False, 0.0, 0.0), first), (real, fusion)
        plan.set_bands(2.0 * W)  # exact in binary: twice the first result, bit for bit
        assert np.array_equal(api.forward(plan, x, batch, length, 2, False, 0.0, 0.0), 2 * first), (real, fusion)
        plan.set_bands(W)


def test_chunk_walk_is_bit_equal_to_the_unbounded_handle(api, monkeypatch):
    """Scratch bytes per frame: bins complex + n_fft reals.  Bounds of 1, 2, 3, 7 and 40 frames against 57 frames in all (19 a row):
    57, 29, 19, 9 and 2 chunks, most of them ending inside a row.  No sum crosses a frame, so every walk is bit-equal.  That the bound is
    honoured is observed through the emulator's allocator (below)."""
    rng = np.random.default_rng(21)
    n, hop, length, batch = 64, 16, 300, 3
    x = np.ascontiguousarray(rng.standard_normal((batch, length)))
    w = truth.hann(n)
    W = cases.mel_bank(n, 12)
    ref = api.make("f64", n, 12, hop)
    ref.set_window_ptr(w.ctypes.data)
    ref.set_bands(W)
    assert ref.describe().startswith("bandspec composed")  # no fused kernel at n_fft = 64
    frames = ref.frames(length)
    assert frames == 19
    P = api.forward(ref, x, batch, length, 2, False, 0.0, 0.0)
    Lg = api.forward(ref, x, batch, length, 1, True, 3.0, 0.5)
    want = truth.band_spectrogram(x, W, n, hop, n, w, "reflect", 2)
    assert np.linalg.norm(P - want) / np.linalg.norm(want) <= cases.tol(ref, "f64")
    per_frame = (n // 2 + 1) * 16 + n * 8
    for k in (1, 2, 3, 7, 40):
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(k * per_frame))
        small = api.make("f64", n, 12, hop)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_window_ptr(w.ctypes.data)
        small.set_bands(W)
        # That more than one chunk runs is observed, not computed: while the emulator's allocator refuses every request above k
        # frames' worth (HIPEMU_MAX_ALLOC), the bounded handle's first call -- the one that sizes its scratch -- succeeds, so its scratch
        # holds at most k of the 57 frames it transforms; a handle without the bound fails the same call for lack of memory.
        unbounded = api.make("f64", n, 12, hop)  # a fresh handle without the bound: its scratch is not sized yet
        unbounded.set_bands(W)
        monkeypatch.setenv("HIPEMU_MAX_ALLOC", str(k * per_frame))
        try:
            first = api.forward(small, x, batch, length, 2, False, 0.0, 0.0)
            with pytest.raises(api.fa.FourierError):
                api.forward(unbounded, x, batch, length, 2, False, 0.0, 0.0)
        finally:
            monkeypatch.delenv("HIPEMU_MAX_ALLOC")
        assert k < batch * frames and np.array_equal(first, P), k
        assert np.array_equal(api.forward(small, x, batch, length, 2, False, 0.0, 0.0), P), k
        assert np.array_equal(api.forward(small, x, batch, length, 1, True, 3.0, 0.5), Lg), k
    # the fused route takes no scratch: the bound does not touch it
    monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", "8")
    one = api.make("f64", 256, 40, 64)
    monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
    big = api.make("f64", 256, 40, 64)
    xx = np.ascontiguousarray(rng.standard_normal((3, 1500)))
    for fusion in (1, 0):  # ... and one frame per chunk on the composed route
        for plan in (one, big):
            plan.set_bands(cases.mel_bank(256))
            plan.set_option("fusion", fusion)
        assert np.array_equal(api.forward(one, xx, 3, 1500, 2, False, 0.0, 0.0), api.forward(big, xx, 3, 1500, 2, False, 0.0, 0.0))


def test_calls_after_reserve_do_not_allocate(fa, api):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(22)
    for fusion in (1, 0):
        n, hop, length = 256, 64, 704
        plan = api.make("f64", n, 40, hop)
        plan.set_bands(cases.mel_bank(n))
        plan.set_option("fusion", fusion)
        plan.reserve(length, 3)
        nf = plan.frames(length)
        x = np.ascontiguousarray(rng.standard_normal((3, length)))
        Y = np.empty((3, nf, 40))
        before = L.fourier_emu_alloc_count()
        for b in (1, 3, 2):
            plan.forward_ptr(x.ctypes.data, Y.ctypes.data, length, b)
            plan.forward_ptr(x.ctypes.data, Y.ctypes.data, length - 64, b, 1, True, 2.0, 1e-3)  # and a shorter row, under the log
        assert L.fourier_emu_alloc_count() == before, fusion


def test_invalid_arguments(fa, api):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_bandspec_{op}_double")  # noqa: E731
    create, fwd, status, opt, reserve, set_bands = (fn(op) for op in ("create", "forward", "last_status", "set_option", "reserve", "set_bands"))
    for bad in ((0, 1, 1, 1, 4), (8, 0, 8, 1, 4), (8, 2, 0, 1, 4), (8, 2, 9, 1, 4), (8, 2, 8, 3, 4), (8, 2, 8, -1, 4), (8, 2, 8, 1, 0),
                (8, 2, 8, 1, 65536)):
        assert not create(*bad, -1), bad
    n, hop, length, bands = 16, 4, 40, 5
    plan = api.make("f64", n, bands, hop)
    h = plan._h
    assert (fn("n_fft")(h), fn("hop")(h), fn("win_length")(h), fn("bins")(h), fn("bands")(h)) == (n, hop, n, n // 2 + 1, bands)
    nf = plan.frames(length)
    assert nf == 11 and fn("frames")(h, 8) == 0 and fn("frames")(h, 9) == 3
    x = np.zeros((2, length))
    Y = np.zeros((2, nf, bands))
    big = np.zeros(4 * Y.size + 4 * x.size)
    # forward before any set_bands
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 0.0, 0.0, None) == INVALID and status(h) == INVALID
    W = np.ascontiguousarray(np.random.default_rng(1).standard_normal((bands, n // 2 + 1)))
    assert set_bands(h, None, None) == INVALID
    assert set_bands(h, W.ctypes.data + 4, None) == INVALID
    for poison in (np.nan, np.inf, -np.inf):
        Wp = W.copy()
        Wp[3, 2] = poison
        assert set_bands(h, Wp.ctypes.data, None) == INVALID and status(h) == INVALID
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 0.0, 0.0, None) == INVALID  # a refused bank is no bank
    assert set_bands(h, W.ctypes.data, None) == 0 and status(h) == 0
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 0.0, 0.0, None) == 0 and status(h) == 0
    Wp = W.copy()
    Wp[0, 0] = np.nan
    assert set_bands(h, Wp.ctypes.data, None) == INVALID  # ... and a refused replacement keeps the bank that was there
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 1, 1, 0.0, 0.0, None) == 0
    for power in (0, 3, -1):
        assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, power, 0, 0.0, 0.0, None) == INVALID and status(h) == INVALID
    # the log: log_mult == 0 ignores the floor; otherwise finite and > 0
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 0.0, -1.0, None) == 0
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 0.0, float("nan"), None) == 0
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 1.0, 1e-10, None) == 0
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, -4.5, 1e-10, None) == 0
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, 1.0, floor, None) == INVALID and status(h) == INVALID
    for mult in (float("nan"), float("inf")):
        assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 2, 2, 0, mult, 1e-3, None) == INVALID
    assert fwd(h, None, Y.ctypes.data, length, 2, 2, 0, 0.0, 0.0, None) == INVALID
    assert fwd(h, x.ctypes.data, None, length, 2, 2, 0, 0.0, 0.0, None) == INVALID
    assert fwd(h, x.ctypes.data + 4, Y.ctypes.data, length, 1, 2, 0, 0.0, 0.0, None) == INVALID   # reals: aligned to 8 bytes
    assert fwd(h, x.ctypes.data, Y.ctypes.data + 4, length, 1, 2, 0, 0.0, 0.0, None) == INVALID
    assert fwd(h, x.ctypes.data + 8, Y.ctypes.data + 8, length - 1, 1, 2, 0, 0.0, 0.0, None) == 0  # ... which is enough, on both sides
    assert fwd(h, x.ctypes.data, Y.ctypes.data, 8, 2, 2, 0, 0.0, 0.0, None) == INVALID            # an invalid length
    assert fwd(h, big.ctypes.data, big.ctypes.data, length, 2, 2, 0, 0.0, 0.0, None) == INVALID   # in place
    assert fwd(h, big.ctypes.data, big.ctypes.data + 8 * length, length, 4, 2, 0, 0.0, 0.0, None) == INVALID  # the output begins inside the input
    assert fwd(h, big.ctypes.data, big.ctypes.data + 16 * length, length, 2, 2, 0, 0.0, 0.0, None) == 0       # adjacent
    assert fwd(h, x.ctypes.data, Y.ctypes.data, length, 0, 2, 0, 0.0, 0.0, None) == 0             # batch 0: a no-op
    assert reserve(h, 8, 1) == INVALID and reserve(h, length, 0) == 0 and reserve(h, length, 2) == 0
    assert fn("set_window")(h, x.ctypes.data + 4, None) == INVALID
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("bandspec composed")  # no fused kernel at n_fft = 16
    # a float32 floor that rounds to zero is refused too
    p32 = api.make("f32", n, bands, hop)
    p32.set_bands(W)
    x32, Y32 = x.astype(np.float32), Y.astype(np.float32)
    f32 = L.fourier_hip_bandspec_forward_float
    assert f32(p32._h, x32.ctypes.data, Y32.ctypes.data, length, 2, 2, 0, 1.0, 1e-30, None) == 0
    assert f32(p32._h, x32.ctypes.data, Y32.ctypes.data, length, 2, 2, 0, 1.0, 1e-60, None) == INVALID
    # the Python layer
    with pytest.raises(fa.FourierError):
        plan.forward_ptr(0, Y.ctypes.data, length, 1)
    with pytest.raises(ValueError):
        fa.BandSpectrogram(16, 4, "f32", 4, 17)
    with pytest.raises(ValueError):
        fa.BandSpectrogram(16, 4, "f32", 4, pad_mode="edge")
    with pytest.raises(ValueError):
        fa.BandSpectrogram(16, 0)
    with pytest.raises(ValueError):
        plan.set_bands(np.zeros((bands, n // 2)))
    with pytest.raises(ValueError):
        plan.set_bands(np.full((bands, n // 2 + 1), np.nan))
    with pytest.raises(TypeError):
        plan.set_bands([[0.0] * (n // 2 + 1)] * bands)
    with pytest.raises(TypeError):
        plan.set_bands(np.zeros((bands, n // 2 + 1), np.complex128))
