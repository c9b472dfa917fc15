"""The delay handle (fourier_hip_delay_*, fourier_amd.Delay) WITHOUT a GPU: the engine sources compiled against the CPU emulation
(tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/delay_truth.py.  The cases, the measure
and the bound (3 x base) are tests/delay_cases.py; the `-m gpu` twin, tests/test_gpu_delay.py, runs the same cases on device buffers
and holds the checks that need device tensors."""
import ctypes

import numpy as np
import pytest

import delay_cases as cases
import delay_truth as truth

INVALID = cases.INVALID


@pytest.fixture(scope="module")
def be():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield cases.HostBackend(fourier_amd)
    _lib._lib = prev
    cases.report("emu")


def test_truth_reproduces_shifts_rolls_and_a_delayed_cosine():
    rng = np.random.default_rng(1)
    n, L = 50, 64
    x = truth.rows(rng, 4, n, np.float64)
    d = np.array([0.0, 3.0, 14.0, 7.0])
    got = truth.delay(x, d, L)
    for r, s in enumerate(d.astype(int)):
        want = np.zeros(n)
        want[s:] = x[r, :n - s]
        assert np.abs(got[r] - want).max() <= 1e-14
    z = truth.rows(rng, 3, n, np.complex128)
    for r, s in enumerate((2.0, -5.0, 1e9 + 3)):
        assert np.abs(truth.delay(z[r:r + 1], np.array([s]), n)[0] - np.roll(z[r], int(s % n))).max() <= 1e-14
    t = np.arange(L)
    c = np.cos(2 * np.pi * 5 * t / L)[None, :]
    assert np.abs(truth.delay(c, np.array([0.3]), L)[0] - np.cos(2 * np.pi * 5 * (t - 0.3) / L)).max() <= 3e-14
    assert np.abs(truth.multiplier(8, [0.5, 3.0])[:, 4] - [0.0, -1.0]).max() <= 1e-16  # the Nyquist bin: cos(pi d)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("i", range(5))
def test_one_launch(be, real, i):
    L, n = cases.ONE_LAUNCH[real][i]
    cases.one_launch(be, real, L, n, weighted=i % 2 == 1)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_no_kernel_at_other_lengths(be, real):
    for n, L, cplx, channels, why in ((1024, 1024, False, 1, "no one-launch kernel for this length"), (65536, 65536, False, 1, "for this length"),
                                      (2048, 2048, True, 1, "complex rows"), (2048, 2048, False, 2, "delay-and-sum")):
        plan, route = cases.make(be, n, L, real, cplx, channels, 1)
        assert route == "composed" and why in plan.describe(), plan.describe()
    if real == "f64":
        plan, route = cases.make(be, 32768, 32768, real, fusion=1)
        assert route == "composed" and "no one-launch kernel" in plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("L", cases.COMPOSED)
def test_composed(be, real, cplx, channels, L):
    cases.composed(be, real, cplx, channels, L)


def test_huge_delays(be):
    cases.huge_delays(be)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_non_finite_delay_or_weight(be, real, fusion):
    cases.non_finite(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion,channels", [(1, 1), (0, 1), (0, 3)])
def test_repetition_and_power_of_two_scaling(be, real, fusion, channels):
    cases.repetition_and_scaling(be, real, fusion, channels)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_integer_delays_shift_and_zero_delay_is_the_input(be, real, fusion):
    cases.integer_delays_shift(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_and_launch_walks(be, monkeypatch, real):
    cases.walks(be, monkeypatch, real)


def test_reserve_then_calls_do_not_allocate(be):
    from fourier_amd import _lib

    lib = _lib.lib()
    lib.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for L, n, cplx, channels, fusion in ((1000, 600, False, 3, 0), (2048, 1501, False, 1, 1), (2048, 1501, False, 1, 0), (255, 255, True, 3, 0), (255, 150, True, 1, 0)):
        plan, _ = cases.make(be, n, L, "f64", cplx, channels, fusion)
        plan.reserve(6)
        x, d, w = cases.inputs(rng, "f64", n, cplx, True)
        out = np.empty((6 // channels, n), x.dtype)
        before = lib.fourier_emu_alloc_count()
        for b in (channels, 6, 3):
            plan.apply_ptr(x.ctypes.data, d.ctypes.data, w.ctypes.data, out.ctypes.data, b)
        assert lib.fourier_emu_alloc_count() == before, (L, cplx, channels, fusion)


def test_invalid_arguments(be):
    from fourier_amd import _lib

    fa = be.fa
    lib = _lib.lib()
    fn = lambda op: getattr(lib, f"fourier_hip_delay_{op}_double")  # noqa: E731
    create, apply, status, opt, reserve = (fn(op) for op in ("create", "apply", "last_status", "set_option", "reserve"))
    n = L = 16
    for bad in ((0, L, 1, 1), (L + 1, L, 1, 1), (n, L, 0, 1), (n, L, 1, 2), (n, L, 1, -1), (n, 1 << 28, 1, 1)):
        assert not create(*bad, -1), bad
    plan = fa.Delay(n, L, "f64", True, 3)
    h = plan._h
    assert (fn("size")(h), fn("length")(h), fn("channels")(h)) == (n, L, 3)
    x, o, d, w = np.zeros((6, n)), np.zeros((2, n)), np.zeros(6), np.ones(6)
    big = np.zeros(16 * x.size)
    X, O, D, W, B = (a.ctypes.data for a in (x, o, d, w, big))
    row = 8 * n
    assert apply(h, X, D, W, O, 6, None) == 0 and status(h) == 0
    assert apply(h, X, D, None, O, 6, None) == 0                       # no weights
    assert apply(h, X, D, W, O, 5, None) == INVALID and status(h) == INVALID  # batch % C
    assert apply(h, X, D, W, O, 0, None) == 0 and status(h) == 0       # batch 0: a no-op
    assert apply(h, None, D, W, O, 6, None) == INVALID and apply(h, X, None, W, O, 6, None) == INVALID
    assert apply(h, X, D, W, None, 6, None) == INVALID
    for k in range(4):  # reals: aligned to 8 bytes
        args = [X, D, W, O]
        args[k] += 4
        assert apply(h, *args, 3, None) == INVALID, k
    assert apply(h, X + 8, D + 8, W + 8, O + 8, 3, None) == 0           # ... an odd real is enough
    assert apply(h, B, D, W, B, 6, None) == INVALID                    # C > 1: never in place
    assert apply(h, B + 2 * row, D, W, B, 6, None) == 0                # the input behind the output: adjacent
    assert apply(h, B + 2 * row - 8, D, W, B, 6, None) == INVALID      # ... one real earlier: inside it
    assert apply(h, B, D, W, B + 6 * row, 6, None) == 0                # the output behind the input: adjacent
    assert apply(h, B, D, W, B + 6 * row - 8, 6, None) == INVALID      # ... it begins inside the input
    assert reserve(h, 0) == 0 and reserve(h, 6) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"fusion", -1) == INVALID
    assert opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID and opt(h, b"weighting", 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("delay composed")  # no kernel at L = 16
    one = fa.Delay(n, L, "f64")  # C == 1: the same buffer is an in-place call, a partial overlap is refused
    assert apply(one._h, B, D, W, B, 6, None) == 0
    assert apply(one._h, B, D, W, B + 8, 6, None) == INVALID and apply(one._h, B + 8, D, W, B, 6, None) == INVALID
    cplan = fa.Delay(n, L, "f64", real_data=False)  # complex values: aligned to 2 * sizeof(T); delays and weights stay reals
    z = np.zeros((3, L), np.complex128)
    Z = z.ctypes.data
    assert apply(cplan._h, Z, D, W, Z + 16 * L, 1, None) == 0 and apply(cplan._h, Z, D + 8, W + 8, Z + 16 * L, 1, None) == 0
    assert apply(cplan._h, Z + 8, D, W, Z + 16 * L, 1, None) == INVALID and apply(cplan._h, Z, D, W, Z + 16 * L + 8, 1, None) == INVALID
    with pytest.raises(fa.FourierError):
        plan.apply_ptr(0, D, W, O, 6)
    with pytest.raises(fa.FourierError):
        plan.set_option("fusion", 7)
    for bad in ((0, 8), (9, 8)):
        with pytest.raises(ValueError):
            fa.Delay(*bad)
    with pytest.raises(ValueError):
        fa.Delay(8, 8, channels=0)
    # the tensor layer refuses everything that is not a device tensor of the right dtype before it looks at shapes
    torch = pytest.importorskip("torch")
    for bad in (x, torch.zeros(6, n), torch.zeros(6, n, dtype=torch.complex64)):
        with pytest.raises(TypeError):
            plan.apply(bad, bad)
        with pytest.raises(TypeError):
            fa.fractional_delay(bad, 1.0)
        with pytest.raises(TypeError):
            fa.delay_and_sum(bad, 1.0)
