"""The cepstrum handle (fourier_hip_cepstrum_*, fourier_amd.Cepstrum) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/cepstrum_truth.py.  The
cases, the measures and the bounds (3 x base for the cepstrum, 6 x base for the minimum-phase row) are tests/cepstrum_cases.py; the
`-m gpu` twin, tests/test_gpu_cepstrum.py, runs the same cases on device buffers and holds the checks that need device tensors."""
import ctypes

import numpy as np
import pytest

import cepstrum_cases as cases
import cepstrum_truth as truth

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


def test_truth_reproduces_the_closed_forms():
    """x = [1, -a]: ln|X| = Re ln(1 - a z^-1), so c[q] = -a^q / (2 q) and the folded cepstrum is that of the minimum-phase row itself;
    the maximum-phase row [-a, 1] has the same magnitude"""
    a, L = 0.5, 2048
    x = np.zeros((1, 8))
    x[0, :2] = 1.0, -a
    c = truth.cepstrum_full(x, L)[0]
    q = np.arange(1, 40)
    assert abs(c[0]) <= 1e-15 and np.abs(c[1:40] + a ** q / (2 * q)).max() <= 1e-15
    assert np.abs(truth.minimum_phase_full(x, L)[0, :8] - x[0]).max() <= 1e-14
    assert np.abs(truth.minimum_phase_full(x[:, ::-1][:, 6:], L)[0, :2] - x[0, :2]).max() <= 1e-14
    assert np.array_equal(truth.fold_weights(6), [1, 2, 2, 1, 0, 0]) and np.array_equal(truth.fold_weights(5), [1, 2, 2, 0, 0])
    assert abs(truth.err(truth.CEPSTRUM, c[None, :40], x, L, 40)) == 0


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("i", range(5))
def test_one_launch(be, monkeypatch, real, mode, i):
    L, n, m = cases.ONE_LAUNCH[real][i]
    spilling = not cases.has_kernel(real, mode, L)  # f32 minimum phase at 2^15: an instance the product leaves out
    if spilling:
        monkeypatch.setenv(cases.SPILLING, "1")
    cases.one_launch(be, real, mode, L, n, m, spilling)


def test_the_instances_left_out_of_the_product(be, monkeypatch):
    """f32 minimum phase at 2^13 and 2^15: composed without the development switch, one launch and within the bound with it"""
    for L in (8192, 32768):
        plan, route = cases.make(be, L, L, L, "f32", truth.MINIMUM_PHASE, 1)
        assert route == "composed" and "no one-launch kernel" in plan.describe(), plan.describe()
    monkeypatch.setenv(cases.SPILLING, "1")
    cases.one_launch(be, "f32", truth.MINIMUM_PHASE, 8192, 5000, 5000, True)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_no_kernel_at_other_lengths(be, real, mode):
    for L in (1024, 65536, 3000) + ((32768,) if real == "f64" else ()):
        plan, route = cases.make(be, L, L, L, real, mode, 1)
        assert route == "composed" and "no one-launch kernel" in plan.describe(), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("L", cases.COMPOSED)
def test_composed(be, real, mode, L):
    cases.composed(be, real, mode, L)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("L,n", [(2048, 1501), (4096, 2049)])
def test_routes_agree(be, real, mode, L, n):
    cases.routes_agree(be, real, mode, L, n)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_known_answers(be, real, fusion):
    cases.known_answers(be, real, fusion)
    cases.magnitude_is_kept(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_floor_on_a_zero_row(be, real, fusion):
    cases.floor_on_a_zero_row(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_floor_whose_square_leaves_the_format(be, real, fusion):
    cases.floor_whose_square_leaves_the_format(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("fusion", [1, 0])
def test_zero_floor_on_a_zero_row_touches_nothing_else(be, real, mode, fusion):
    cases.zero_floor_on_a_zero_row(be, real, mode, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("fusion", [1, 0])
def test_log_mult(be, real, mode, fusion):
    cases.log_mult_half(be, real, mode, fusion)


def test_minimum_phase_half_against_scipy(be):
    """scipy.signal.minimum_phase(firwin(101, 0.3), "homomorphic", n_fft=8192, half=...): relative 1e-5 at f64 in spite of the two
    documented deviations (the floor, quefrency L/2); scipy keeps (n + 1) / 2 taps"""
    signal = pytest.importorskip("scipy.signal")
    h = signal.firwin(101, 0.3)
    for half in (True, False):
        want = signal.minimum_phase(h, method="homomorphic", n_fft=8192, half=half)
        plan, _ = cases.make(be, 101, 8192, len(want), "f64", truth.MINIMUM_PHASE, 0)
        got = cases.run(be, plan, h[None, :], 0.5 if half else 1.0)[0]
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"cepstrum f64 against scipy half={half}: relative {rel:.3g}")
        assert rel <= 1e-5, (half, rel)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_chunk_and_launch_walks(be, monkeypatch, real, mode):
    cases.walks(be, monkeypatch, real, mode)


def test_reserve_then_calls_do_not_allocate(be):
    from fourier_amd import _lib

    lib = _lib.lib()
    lib.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for L, n, mode, fusion in ((1000, 600, 1, 0), (2048, 1501, 1, 1), (2048, 1501, 0, 0), (255, 255, 0, 0)):
        plan, _ = cases.make(be, n, L, n, "f64", mode, fusion)
        plan.reserve(6)
        x = truth.rows(rng, 6, n, np.float64)
        out = np.empty((6, n))
        before = lib.fourier_emu_alloc_count()
        for b in (1, 6, 3):
            plan.apply_ptr(x.ctypes.data, out.ctypes.data, b)
        assert lib.fourier_emu_alloc_count() == before, (L, mode, fusion)


def test_invalid_arguments(be):
    from fourier_amd import _lib

    fa = be.fa
    lib = _lib.lib()
    fn = lambda op: getattr(lib, f"fourier_hip_cepstrum_{op}_double")  # noqa: E731
    create, apply, status, opt, reserve = (fn(op) for op in ("create", "apply", "last_status", "set_option", "reserve"))
    n = L = 16
    # (size, length, outputs, mode): n == 0, n > L, m == 0, m > L, a mode that is not 0 or 1, rows above 2^31 bytes
    for bad in ((0, L, 1, 0), (L + 1, L, 1, 0), (n, L, 0, 0), (n, L, L + 1, 1), (n, L, n, 2), (n, L, n, -1), (n, 1 << 28, n, 0)):
        assert not create(*bad, -1), bad
    plan = fa.Cepstrum(n, L, "f64", 8, 1)
    h = plan._h
    assert (fn("size")(h), fn("length")(h), fn("outputs")(h), fn("mode")(h)) == (n, L, 8, 1)
    x, o = np.ones((6, n)), np.zeros((6, 8))
    big = np.ones(16 * x.size)
    X, O, B = (a.ctypes.data for a in (x, o, big))
    row = 8 * n
    assert apply(h, X, O, 6, 1.0, 0.0, None) == 0 and status(h) == 0
    assert apply(h, X, O, 6, 0.0, 0.0, None) == INVALID and status(h) == INVALID   # log_mult == 0
    assert apply(h, X, O, 0, 1.0, 0.0, None) == 0 and status(h) == 0               # batch 0: a no-op
    for lm, fl in ((np.nan, 0.0), (np.inf, 0.0), (-np.inf, 0.0), (1.0, -1e-30), (1.0, np.nan), (1.0, np.inf)):
        assert apply(h, X, O, 6, lm, fl, None) == INVALID, (lm, fl)
    assert apply(h, X, O, 6, -2.5, 3.0, None) == 0                                 # any other finite pair
    assert apply(h, None, O, 6, 1.0, 0.0, None) == INVALID and apply(h, X, None, 6, 1.0, 0.0, None) == INVALID
    assert apply(h, X + 4, O, 3, 1.0, 0.0, None) == INVALID and apply(h, X, O + 4, 3, 1.0, 0.0, None) == INVALID  # reals: 8 bytes
    assert apply(h, X + 8, O + 8, 3, 1.0, 0.0, None) == 0                          # ... an odd real is enough
    assert apply(h, B, B, 6, 1.0, 0.0, None) == INVALID                            # m != n: never in place
    assert apply(h, B + 3 * row, B, 6, 1.0, 0.0, None) == 0                        # the input behind the output (6 rows of 8): adjacent
    assert apply(h, B + 3 * row - 8, B, 6, 1.0, 0.0, None) == INVALID              # ... one real earlier: inside it
    assert apply(h, B, B + 6 * row, 6, 1.0, 0.0, None) == 0                        # the output behind the input: adjacent
    assert apply(h, B, B + 6 * row - 8, 6, 1.0, 0.0, None) == INVALID              # ... it begins inside the input
    assert reserve(h, 0) == 0 and reserve(h, 6) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"fusion", -1) == INVALID
    assert opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID and opt(h, b"weighting", 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("cepstrum composed")  # no kernel at L = 16
    same = fa.Cepstrum(n, L, "f64")  # m == n: the same buffer is an in-place call, a partial overlap is refused
    assert apply(same._h, B, B, 6, 1.0, 0.0, None) == 0
    assert apply(same._h, B, B + 8, 6, 1.0, 0.0, None) == INVALID and apply(same._h, B + 8, B, 6, 1.0, 0.0, None) == INVALID
    with pytest.raises(fa.FourierError):
        plan.apply_ptr(0, O, 6)
    with pytest.raises(fa.FourierError):
        plan.apply_ptr(X, O, 6, log_mult=0.0)
    with pytest.raises(fa.FourierError):
        plan.set_option("fusion", 7)
    for bad in ((0, 8), (9, 8), (8, 8, "f32", 0), (8, 8, "f32", 9), (8, 8, "f32", 8, 2)):
        with pytest.raises(ValueError):
            fa.Cepstrum(*bad)
    # the tensor layer refuses everything that is not a device tensor of the right dtype before it looks at shapes
    torch = pytest.importorskip("torch")
    for bad in (x, torch.zeros(6, n), torch.zeros(6, n, dtype=torch.complex64)):
        with pytest.raises(TypeError):
            plan.apply(bad)
        with pytest.raises(TypeError):
            fa.real_cepstrum(bad)
        with pytest.raises(TypeError):
            fa.minimum_phase(bad)
