"""The resampling handle (fourier_hip_resample_*, fourier_amd.Resample) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/resample_truth.py (the
definition of include/fourier.h in f64 numpy on the rounded input), which is itself cross-checked against scipy.signal.resample here.
The `-m gpu` twin is tests/test_gpu_resample.py, which also holds the tensor layer.

Inputs: seeded white Gaussian rows, batch 3; windows: seeded uniform values in [0.5, 1.5].  Tolerance, relative L2 over the whole output:
2 x base, base the single-transform figure tests/test_gpu_real.py grants -- f32 2e-6 (4e-6 if either plan is a Bluestein plan), f64
1e-13 (1e-11 likewise) -- because two transforms in T contribute (the rule of tests/test_gpu_hilbert.py).  The window is bounded by 1.5
and adds one rounding: no allowance of its own.  Every figure is printed before it is asserted; the worst of a run, as a fraction of its
bound, is printed at the end."""
import ctypes

import numpy as np
import pytest

import resample_truth as truth
from helpers import rel_l2

SENTINEL = 77.0
WORST = {}
PAIRS = ((1, 1), (1, 5), (5, 1), (2, 1), (1, 2), (2, 4), (4, 2), (3, 2), (8, 8), (16, 12), (12, 16), (15, 10), (10, 15), (9, 7), (7, 9),
         (255, 256), (480, 441), (441, 480))
SCIPY_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 30, 31)


def test_truth_is_scipy_signal_resample():
    """N and M over SCIPY_SIZES, real and complex rows, with and without a window, at 1e-12 relative L2; complex rows with M == 2 < N (the
    documented exception) are left out, nothing else is"""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(11)
    worst = 0.0
    for n in SCIPY_SIZES:
        for m in SCIPY_SIZES:
            for complex_rows in (False, True):
                if complex_rows and m == 2 < n:
                    continue
                for windowed in (False, True):
                    x = truth.rows(rng, 3, n, np.float64, complex_rows)
                    w = truth.window(rng, n, np.float64) if windowed else None
                    want = signal.resample(x, m, axis=-1, window=w)
                    err = rel_l2(truth.resample(x, m, w), want)
                    worst = max(worst, err)
                    assert err <= 1e-12, (n, m, complex_rows, windowed, err)
    print(f"resample truth against scipy: worst relative L2 {worst:.3g}")


def test_truth_of_complex_rows_with_zero_imaginary_part_is_the_truth_of_real_rows():
    """... the exception included: M == 2 < N.  Without a window and with a symmetric one, W[k] = W[N-k] (an asymmetric window is folded
    for real rows and makes complex rows complex)"""
    rng = np.random.default_rng(12)
    for n in SCIPY_SIZES:
        for m in SCIPY_SIZES:
            x = truth.rows(rng, 2, n, np.float64)
            w = truth.window(rng, n, np.float64)
            w = (w + np.roll(w[::-1], 1)) / 2
            for win in (None, w):
                z = truth.resample(x.astype(np.complex128), m, win)
                assert rel_l2(z, truth.resample(x, m, win).astype(np.complex128)) <= 1e-13, (n, m)


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
        print(f"resample emu worst err / bound {key}: {v:.3g}")


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return 2 * base


def routes(plan):
    """the routes of a handle as (name, "fusion" value)"""
    if not plan.real_input:
        return (("complex", 0),)
    if plan.size_in() % 2 == 0 and plan.size_out() % 2 == 0:
        return (("real fused untangle", 1), ("real composed", 0))
    return (("real composed", 0),)


def select(plan, name, fusion):
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith(f"resample {name}: "), plan.describe()


def run(plan, x, first=1):
    """forward_ptr into a buffer whose output starts on element `first` (1: an odd element) with sentinels on both sides; checks them and
    that the input is unmodified"""
    batch = x.shape[0]
    bx = x.tobytes()
    count = batch * plan.size_out()
    buf = np.full(count + first + 2, SENTINEL, x.dtype)
    out = buf[first:first + count]
    plan.forward_ptr(x.ctypes.data, out.ctypes.data, batch)
    assert np.all(buf[:first] == SENTINEL) and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
    assert x.tobytes() == bx, "forward modified its input"
    return out.reshape(batch, plan.size_out()).copy()


def note(real, what, route, err, bound, shape):
    print(f"{what} {real} {shape[0]}->{shape[1]} {route}: err {err:.3g} bound {bound:.3g}")
    key = (real, what, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, (real, what, route, shape, err, bound)


def check(fa, real, n, m, complex_rows, batch=3):
    """every route of the shape with the describe string asserted, without and with a window, against the truth; the two real routes
    within twice the bound of each other"""
    rng = np.random.default_rng(100000 * complex_rows + 1000 * n + m)
    x = truth.rows(rng, batch, n, rdt(real), complex_rows)
    w = truth.window(rng, n, rdt(real))
    plan = fa.Resample(n, m, real, real_input=not complex_rows)
    assert plan.size_in() == n and plan.size_out() == m
    assert plan.describe().startswith(f"resample {routes(plan)[0][0]}: "), plan.describe()  # the default: the fused route where it exists
    if complex_rows or n % 2 or m % 2:  # "fusion" = 1 is accepted and changes nothing
        before = plan.describe()
        plan.set_option("fusion", 1)
        assert plan.describe() == before and not before.startswith("resample real fused")
    for windowed in (False, True):
        want = truth.resample(x, m, w if windowed else None)
        what = "windowed" if windowed else "plain"
        got = {}
        for name, fusion in routes(plan):
            select(plan, name, fusion)
            plan.set_window_ptr(w.ctypes.data if windowed else None)
            y = run(plan, x)
            bound = tol(plan, real)
            note(real, what, name, rel_l2(y, want), bound, (n, m))
            got[name] = y, bound
        if len(got) == 2:
            (a, ba), (b, bb) = got.values()
            note(real, what, "real routes", rel_l2(a, b), 2 * max(ba, bb), (n, m))


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("complex_rows", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_shapes(fa, real, complex_rows, pair):
    check(fa, real, pair[0], pair[1], complex_rows)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_clearing_the_window_restores_the_unwindowed_result_bit_for_bit(fa, real):
    n, m = 480, 441
    rng = np.random.default_rng(3)
    for complex_rows in (False, True):
        x = truth.rows(rng, 3, n, rdt(real), complex_rows)
        w = truth.window(rng, n, rdt(real))
        plan = fa.Resample(n, m, real, real_input=not complex_rows)
        plain = run(plan, x)
        plan.set_window_ptr(w.ctypes.data)
        windowed = run(plan, x)
        assert not np.array_equal(windowed, plain)
        w[...] = 0  # the handle keeps its own copy
        assert np.array_equal(run(plan, x), windowed)
        plan.set_window_ptr(None)
        assert np.array_equal(run(plan, x), plain), (real, complex_rows)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(fa, real, monkeypatch):
    """5 rows under a bound of two rows of scratch (3 chunks): bit-equal to the unbounded handle, on both real routes and the complex one"""
    rng = np.random.default_rng(7)
    elem = 8 if real == "f32" else 16
    for n, m in ((16, 12), (255, 256)):
        for complex_rows in (False, True):
            x = truth.rows(rng, 5, n, rdt(real), complex_rows)
            per = n * elem if complex_rows else (n // 2 + 1 + m // 2 + 1) * elem  # a row's spectrum, or its two half spectra
            whole = fa.Resample(n, m, real, real_input=not complex_rows)
            monkeypatch.setenv("FOURIER_RESAMPLE_SCRATCH_BYTES", str(2 * per + 8))
            small = fa.Resample(n, m, real, real_input=not complex_rows)
            monkeypatch.delenv("FOURIER_RESAMPLE_SCRATCH_BYTES")
            want = truth.resample(x, m)
            for name, fusion in routes(whole):
                select(whole, name, fusion)
                select(small, name, fusion)
                a, b = run(whole, x), run(small, x)
                assert np.array_equal(a, b), (real, n, m, name)
                note(real, "chunks", name, rel_l2(b, want), tol(small, real), (n, m))


def test_reserve_then_calls_do_not_allocate_and_repeat_bit_equal(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for n, m in ((480, 441), (16, 12), (255, 256)):
        for complex_rows in (False, True):
            plan = fa.Resample(n, m, "f64", real_input=not complex_rows)
            for name, fusion in routes(plan):
                select(plan, name, fusion)
                plan.reserve(5)
                x = truth.rows(rng, 5, n, np.float64, complex_rows)
                y = np.empty((5, m), x.dtype)
                before = L.fourier_emu_alloc_count()
                for b in (1, 5, 3):
                    plan.forward_ptr(x.ctypes.data, y.ctypes.data, b)
                assert L.fourier_emu_alloc_count() == before, (n, m, name)
                assert np.array_equal(run(plan, x), run(plan, x)), (n, m, name)


def test_tensor_layer_refuses_what_is_not_a_device_tensor(fa):
    torch = pytest.importorskip("torch")
    plan = fa.Resample(16, 12, "f64")
    for bad in (np.zeros((2, 16)), torch.zeros(2, 16, dtype=torch.float64)):
        with pytest.raises(TypeError):
            plan.forward(bad)
        with pytest.raises(TypeError):
            fa.resample(bad, 12)
        with pytest.raises(TypeError):
            plan.set_window(bad)
