"""N-D convolution with a prepared filter bank (fourier_hip_convnd_*, fourier_amd.FftConvNd) WITHOUT a GPU: the engine sources
compiled against the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product -- the cases of
tests/convnd_cases.py, which the `-m gpu` twin tests/test_gpu_convnd.py runs on device buffers, against tests/convnd_truth.py.
Measure, bounds and shapes are stated in tests/convnd_cases.py.  Here also: the argument checks of the C ABI that need a handle, the
allocation-free property after reserve (through the emulator's allocation counter), next_fast_len, and the truth's linear windows
against scipy."""
import ctypes

import numpy as np
import pytest

import convnd_cases as cases
import convnd_truth as truth
from helpers import rel_l2

REALS = ["f32", "f64"]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev
    cases.report("emu")


@pytest.fixture
def be(fa, monkeypatch):
    return cases.HostBackend(fa, monkeypatch)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape", cases.MID_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_mid_kernel_edges_on_both_routes(be, real, shape):
    cases.mid_edges(be, real, shape)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_banks(be, real, fusion):
    cases.banks(be, real, fusion)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_windows(be, real, fusion):
    cases.windows(be, real, fusion)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_linear_modes_against_scipy(be, real, fusion):
    cases.linear_modes(be, real, fusion)


def test_the_truths_linear_windows_are_scipys():
    rng = np.random.default_rng(3)
    for a, k in cases.LINEAR:
        x, h = rng.standard_normal((2,) + a), rng.standard_normal((2,) + k)
        shape = tuple(n + m - 1 for n, m in zip(a, k))
        for mode in cases.MODES:
            fst, size = truth.linear_window(a, k, mode)
            assert rel_l2(truth.window(truth.circular(x, h, shape), fst, size), truth.scipy_linear(x, h, mode)) <= 1e-14, (a, k, mode)
            # scipy's correlate for real data is the convolution with the taps flipped along every dimension
            assert rel_l2(truth.scipy_linear(x, h[:, ::-1, ::-1], mode), truth.scipy_linear(x, h, mode, correlate=True)) <= 1e-14


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("items", [2, 1])
def test_scratch_walk(be, real, fusion, items):
    for shape, windowed in (((4, 6), False), ((3, 8), True), ((2, 5, 6), True), ((4, 7), True)):
        if not fusion or cases.has_fused(shape):
            cases.scratch_walk(be, real, shape, fusion, items, windowed)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("fusion", [1, 0])
def test_launch_walk(be, real, fusion):
    for shape in ((4, 6), (2, 600), (2, 3, 2, 8)):  # (2, 600): a half spectrum beyond one workgroup, so the product sweep's N-D twin
        for batch in range(3, 8):
            cases.launch_walk(be, real, shape, fusion, batch, True)


@pytest.mark.parametrize("real", REALS)
def test_argument_checks(be, real):
    cases.argument_checks(be, real)


def test_create_and_the_null_handle(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    sizes = lambda *v: (ctypes.c_size_t * len(v))(*v)  # noqa: E731
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(L, f"fourier_hip_convnd_{op}_{s}")  # noqa: E731
        assert not fn("create")(1, sizes(16), -1)            # rank 1 is fourier_hip_conv_*
        assert not fn("create")(5, sizes(2, 2, 2, 2, 2), -1)
        assert not fn("create")(0, sizes(2), -1)
        assert not fn("create")(2, None, -1)
        assert not fn("create")(2, sizes(4, 0), -1)
        assert not fn("create")(3, sizes(0, 4, 4), -1)
        h = fn("create")(3, sizes(2, 3, 4), -1)
        assert h and fn("rank")(h) == 3 and fn("filters")(h) == 0
        out = sizes(0, 0, 0)
        assert fn("shape")(h, out) == 0 and list(out) == [2, 3, 4]
        assert fn("shape")(h, None) == cases.INVALID
        assert fn("set_option")(h, None, 1) == cases.INVALID
        assert fn("set_window")(h, None, out, out) == cases.INVALID and fn("last_status")(h) == cases.INVALID
        assert fn("set_filters")(h, 16, None, 1, 0, None) == cases.INVALID
        assert fn("reserve")(h, 3) == 0 and fn("last_status")(h) == 0
        fn("destroy")(h)
    with pytest.raises(ValueError):
        fa.FftConvNd((16,), "f32")
    with pytest.raises(ValueError):
        fa.FftConvNd((2, 2, 2, 2, 2), "f32")
    with pytest.raises(ValueError):
        fa.FftConvNd((4, 0), "f64")


def test_calls_after_reserve_do_not_allocate(be):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(30)
    for shape in ((4, 6), (5, 8), (3, 4, 10), (4, 7), (40, 96)):
        for fusion in cases.routes(shape):
            plan, route = cases.make(be, shape, "f64", fusion)
            cases.set_filters(be, plan, cases.rand(rng, (2,) + tuple(min(3, n) for n in shape), "f64"))
            a = tuple(max(1, n - 1) for n in shape)
            plan.reserve(5)
            x, xa = cases.rand(rng, (5,) + shape, "f64"), cases.rand(rng, (5,) + a, "f64")
            y = np.empty_like(x)
            before = L.fourier_emu_alloc_count()
            for b in (1, 5, 2):
                plan.set_window()
                plan.apply_ptr(x.ctypes.data, y.ctypes.data, b)
                plan.apply_ptr(y.ctypes.data, y.ctypes.data, b)
                plan.set_window(a, None, a)
                plan.apply_ptr(xa.ctypes.data, y.ctypes.data, b, 1)
            assert L.fourier_emu_alloc_count() == before, (shape, route)


def test_next_fast_len():
    import fourier_amd as fa

    def smooth(m):
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        return m == 1

    for n in list(range(1, 300)) + [1000, 1025, 2030, 4097, 65537]:
        for even in (False, True):
            m = fa.next_fast_len(n, even)
            assert m >= n and smooth(m) and not (even and m % 2)
            assert not any(smooth(c) and not (even and c % 2) for c in range(n, m)), (n, even, m)
    assert [fa.next_fast_len(n) for n in (1, 11, 13, 97, 1025)] == [1, 12, 14, 98, 1029]
    assert fa.next_fast_len(1025, even=True) == 1050 and fa.next_fast_len(1, even=True) == 2
