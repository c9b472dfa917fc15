"""The cross-correlation handle (fourier_hip_xcorr_*, fourier_amd.CrossCorrelation) WITHOUT a GPU: the engine sources compiled against
the CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/xcorr_truth.py (f64
numpy on the rounded inputs).  The `-m gpu` twin is tests/test_gpu_xcorr.py, which also holds the checks that need device tensors.

The one-launch table of the product holds only the kernels that run without scratch memory (f64, no weighting).  The development
switch FOURIER_XCORR_SPILLING, read at create by the emulator build and the experiments library, admits the others: the tests of the
one-launch route create their handles under it, so that every instance of the kernel is checked; test_one_launch_table holds the
product's table.

Measure: ||got - want_window||_2 / ||want over all L lags||_2 (rigorous for any window; rel_l2 when lags == L).  base is the
single-transform figure of tests/test_gpu_real.py: f32 2e-6 (4e-6 on a Bluestein plan), f64 1e-13 (1e-11 on a Bluestein plan).
  no weighting, white rows:  4 x base -- one base per contributing transform (two inputs, one inverse) plus one for the untangle,
                             the rule by which tests/test_gpu_conv.py takes 3 x;
  PHAT, spike rows:          base x (sqrt(2 (kx^2 + ky^2)) + 1), kx, ky = xcorr_truth.kappa: each bin's phasor error is
                             |dX_k| / |X_k| + |dY_k| / |Y_k|, the inverse adds one base; kx, ky <= 3 is asserted first (a condition on
                             the inputs), and argmax_j out == d - lag_first in every row.
Every figure is printed before it is asserted; the worst err / bound per (precision, weighting, route) is printed at module end."""
import ctypes

import numpy as np
import pytest

import xcorr_truth as truth

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, weighting, route) -> the largest err / bound seen
DELAY = 2    # of the spike rows: inside every window below
COMPOSED_ONLY = (1, 2, 3, 7, 16, 100, 255, 1000, 1001, 1031)


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
        print(f"xcorr emu worst err / bound {key}: {v:.3g}")


def dt(real, cplx=False):
    return {("f32", False): np.float32, ("f64", False): np.float64, ("f32", True): np.complex64, ("f64", True): np.complex128}[(real, cplx)]


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def has_kernel(real, L):
    return L in (2048, 4096, 8192, 16384) or (L == 32768 and real == "f32")


def windows(L, n):
    """(lag_first, lags): the whole row, the full linear window where it fits, a short centred one, one that wraps past lag L - 1"""
    w = [(0, L), (-3, 7), (L - 2, 6)]
    if 2 * n - 1 <= L:
        w.insert(1, (-(n - 1), 2 * n - 1))
    return w


def make(fa, monkeypatch, n, L, first, lags, real, cplx=False, phat=False, fusion=0):
    """a handle created under the development switch that admits every one-launch instance"""
    monkeypatch.setenv("FOURIER_XCORR_SPILLING", "1")
    try:
        plan = fa.CrossCorrelation(n, L, first, lags, real, not cplx)
    finally:
        monkeypatch.delenv("FOURIER_XCORR_SPILLING")
    assert (plan.size(), plan.length(), plan.lags()) == (n, L, lags)
    default = "one-launch" if not cplx and has_kernel(real, L) else "composed"  # (the switch admits every instance; no weighting yet)
    assert plan.describe().startswith(f"xcorr {default}: "), plan.describe()
    plan.set_option("weighting", int(phat))
    plan.set_option("fusion", fusion)
    route = "one-launch" if fusion and not cplx and has_kernel(real, L) else "composed"
    assert plan.describe().startswith(f"xcorr {route}: "), plan.describe()
    return plan, route


def run(plan, x, y, first=1):
    """correlate_ptr into a buffer whose output starts on element `first` (1: an odd element) with sentinels on both sides; checks them
    and that the inputs are unmodified"""
    batch = x.shape[0]
    bx, by = x.tobytes(), y.tobytes()
    count = batch * plan.lags()
    buf = np.full(count + first + 2, SENTINEL, x.dtype)
    out = buf[first:first + count]
    plan.correlate_ptr(x.ctypes.data, y.ctypes.data, out.ctypes.data, batch)
    assert np.all(buf[:first] == SENTINEL) and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
    assert x.tobytes() == bx and y.tobytes() == by, "correlate modified an input"
    return out.reshape(batch, plan.lags()).copy()


def note(real, weighting, route, what, err, bound):
    print(f"xcorr {real} {weighting} {route} {what}: err {err:.3g} bound {bound:.3g}")
    key = (real, weighting, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, (real, weighting, route, what, err, bound)


def check(fa, monkeypatch, real, L, n, batch, cplx=False, fusions=(1, 0)):
    """every window and both weightings on the routes of `fusions`, against the truth; the routes within 2 x the larger bound of each
    other; the PHAT peak at the delay"""
    rng = np.random.default_rng(1000 * batch + L + n)
    for phat in (False, True):
        if phat:
            x, y = truth.spike_rows(rng, batch, n, DELAY if n > 2 * DELAY else 0, dt(real, cplx))
            kx, ky = truth.kappa(x, L), truth.kappa(y, L)
            assert kx <= 3 and ky <= 3, (kx, ky)  # a condition on the inputs
        else:
            x, y = truth.rows(rng, batch, n, dt(real, cplx)), truth.rows(rng, batch, n, dt(real, cplx))
        d = DELAY if n > 2 * DELAY else 0
        want = truth.full(x, y, L, phat)
        for first, lags in windows(L, n) if L >= 8 else [(0, L)]:
            got = {}
            for fusion in fusions:
                plan, route = make(fa, monkeypatch, n, L, first, lags, real, cplx, phat, fusion)
                bound = base(plan, real) * ((np.sqrt(2 * (kx * kx + ky * ky)) + 1) if phat else 4)
                out = run(plan, x, y)
                name = "phat" if phat else "none"
                note(real, name, route, f"L={L} n={n} window=({first}, {lags}) batch={batch}", truth.window_err(out, want, first, lags), bound)
                if phat and (d - first) % L < lags:
                    assert np.all(np.argmax(np.abs(out), axis=-1) == (d - first) % L), (real, L, n, first, lags, route)
                got[route] = out, bound
            if len(got) == 2:
                diff = np.linalg.norm(got["one-launch"][0] - got["composed"][0]) / np.linalg.norm(want)
                note(real, "phat" if phat else "none", "routes", f"L={L} n={n} window=({first}, {lags})", diff,
                     2 * max(got["one-launch"][1], got["composed"][1]))


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("L", [2048, 4096, 16384, 32768])
def test_both_routes(fa, monkeypatch, real, L):
    if L == 32768 and real == "f64":  # no f64 kernel of that length: "fusion" = 1 stays on the composed route
        plan, route = make(fa, monkeypatch, L, L, 0, L, real, fusion=1)
        assert route == "composed" and "no one-launch kernel" in plan.describe()
        return
    for i, n in enumerate((L, L // 2) + ((1000,) if L == 2048 else ())):
        check(fa, monkeypatch, real, L, n, (5, 3)[i % 2])
    if L <= 4096:  # ... and each n with the other batch
        check(fa, monkeypatch, real, L, L, 3)
        check(fa, monkeypatch, real, L, L // 2, 5)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_one_launch_table(fa, real):
    """without the development switch, as in the product: only the kernels without scratch memory -- f64, no weighting"""
    for L in (2048, 16384):
        plan = fa.CrossCorrelation(L // 2, L, -3, 7, real)
        for phat in (0, 1):
            plan.set_option("weighting", phat)
            plan.set_option("fusion", 1)
            if real == "f64" and not phat:
                assert plan.describe().startswith("xcorr one-launch: "), plan.describe()
            else:
                assert plan.describe().startswith("xcorr composed: ") and "no one-launch kernel" in plan.describe(), plan.describe()
            plan.set_option("fusion", 0)
            assert plan.describe().startswith("xcorr composed: ")
        plan = fa.CrossCorrelation(L // 2, L, -3, 7, real)  # the default: the one-launch route where it exists
        assert plan.describe().startswith("xcorr one-launch: " if real == "f64" else "xcorr composed: "), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L", COMPOSED_ONLY)
def test_composed_sizes(fa, monkeypatch, real, cplx, L):
    for i, n in enumerate(sorted({L, (L + 1) // 2})):
        check(fa, monkeypatch, real, L, n, (3, 5)[i % 2], cplx, fusions=(0,))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_complex_rows_have_no_one_launch_route(fa, monkeypatch, real):
    plan, route = make(fa, monkeypatch, 2048, 2048, 0, 2048, real, cplx=True, fusion=1)
    assert route == "composed" and "complex rows" in plan.describe()
    check(fa, monkeypatch, real, 2048, 1024, 3, cplx=True, fusions=(1,))


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_x_is_y_is_the_autocorrelation(fa, monkeypatch, real, fusion):
    rng = np.random.default_rng(3)
    for L, n, cplx in ((2048, 1000, False), (255, 128, False), (255, 128, True)):
        x = truth.rows(rng, 3, n, dt(real, cplx))
        plan, route = make(fa, monkeypatch, n, L, -(n - 1), 2 * n - 1, real, cplx, False, fusion)
        out = run(plan, x, x)
        note(real, "none", route, f"autocorrelation L={L} n={n}", truth.window_err(out, truth.full(x, x, L), -(n - 1), 2 * n - 1), 4 * base(plan, real))
        assert np.array_equal(out, run(plan, x, x.copy())), "x is y differs from a copy of x as y"


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_all_zero_row_under_phat_gives_exact_zeros(fa, monkeypatch, real, fusion):
    rng = np.random.default_rng(4)
    for L, n in ((2048, 1024), (100, 100)):
        x, y = truth.spike_rows(rng, 3, n, DELAY, dt(real))
        x[1] = 0
        y[2] = 0
        plan, _ = make(fa, monkeypatch, n, L, 0, L, real, False, True, fusion)
        out = run(plan, x, y)
        assert np.all(np.isfinite(out)) and np.all(out[1:] == 0) and np.any(out[0] != 0)
    if fusion == 0:
        z = np.zeros((2, 16), dt(real, True))
        plan, _ = make(fa, monkeypatch, 16, 16, 0, 16, real, True, True, 0)
        assert np.all(run(plan, z, z) == 0)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("route", ["one-launch", "composed"])
def test_power_of_two_scaling(fa, monkeypatch, real, route):
    """x * 2^20, y * 2^-30: the unweighted output is bit-equal to 2^-10 x the unscaled result, the PHAT output bit-identical.  The
    composed route transforms the rows apart; the one-launch kernel, which transforms x + iy as one row, balances them by powers of two
    first.  The scaled result is also within the bound of the truth: neither row is lost to the other."""
    n = L = 2048
    rng = np.random.default_rng(5)
    x, y = truth.spike_rows(rng, 3, n, DELAY, dt(real))
    xs, ys = (x * 2.0 ** 20).astype(x.dtype), (y * 2.0 ** -30).astype(y.dtype)
    for phat in (False, True):
        plan, got = make(fa, monkeypatch, n, L, 0, L, real, False, phat, int(route == "one-launch"))
        assert got == route
        plain, scaled = run(plan, x, y), run(plan, xs, ys)
        want = truth.full(xs, ys, L, phat)
        bound = base(plan, real) * (np.sqrt(2 * (truth.kappa(x, L) ** 2 + truth.kappa(y, L) ** 2)) + 1 if phat else 4)
        note(real, "phat" if phat else "none", route, "scaled rows", truth.window_err(scaled, want, 0, L), bound)
        assert np.array_equal(scaled, plain if phat else (plain * 2.0 ** -10).astype(plain.dtype)), (real, route, phat)


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("phat", [False, True])
def test_f32_bases_that_are_only_4_byte_aligned(fa, monkeypatch, fusion, phat):
    """the element-wise loads and stores of the one-launch kernel (and the composed route on the same pointers), for x, y and out:
    bit-equal to the aligned call"""
    L, n, batch = 2048, 1024, 3
    rng = np.random.default_rng(6)
    x, y = truth.spike_rows(rng, batch, n, DELAY, np.float32)

    def shifted(v):
        holder = np.zeros(v.size + 1, np.float32)
        s = holder[1:].reshape(v.shape)
        s[...] = v
        assert v.ctypes.data % 8 == 0 and s.ctypes.data % 8 == 4
        return s

    for first, lags in ((0, L), (-(n - 1), 2 * n - 2), (-4, 8)):
        plan, _ = make(fa, monkeypatch, n, L, first, lags, "f32", False, phat, fusion)
        aligned = run(plan, x, y, first=2)
        for xx, yy, o in ((shifted(x), y, 2), (x, shifted(y), 2), (x, y, 1), (shifted(x), shifted(y), 1)):
            assert np.array_equal(run(plan, xx, yy, first=o), aligned), (first, lags)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(fa, real, monkeypatch):
    """5 rows in 3 chunks of two under FOURIER_XCORR_SCRATCH_BYTES: bit-equal to one chunk"""
    rng = np.random.default_rng(7)
    rs, cs = (4, 8) if real == "f32" else (8, 16)
    for L, n, cplx in ((255, 128, False), (2048, 1024, False), (255, 128, True)):
        x, y = truth.rows(rng, 5, n, dt(real, cplx)), truth.rows(rng, 5, n, dt(real, cplx))
        per = 2 * L * cs if cplx else 2 * (L // 2 + 1) * cs + 3 * L * rs  # the scratch of one row pair (xcorr_plan.h)
        for phat in (False, True):
            for first, lags in ((0, L), (-3, 7)):
                whole, _ = make(fa, monkeypatch, n, L, first, lags, real, cplx, phat)
                monkeypatch.setenv("FOURIER_XCORR_SCRATCH_BYTES", str(2 * per + 8))
                small, _ = make(fa, monkeypatch, n, L, first, lags, real, cplx, phat)
                monkeypatch.delenv("FOURIER_XCORR_SCRATCH_BYTES")
                a, b = run(whole, x, y), run(small, x, y)
                assert np.array_equal(a, b), (real, L, cplx, phat, first)


def test_reserve_then_calls_do_not_allocate_and_repeat_bit_equal(fa, monkeypatch):
    from fourier_amd import _lib

    lib = _lib.lib()
    lib.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for L, n, cplx in ((1000, 500, False), (2048, 1024, False), (255, 255, True)):
        for fusion in (1, 0):
            plan, _ = make(fa, monkeypatch, n, L, -3, 7, "f64", cplx, False, fusion)
            plan.reserve(5)
            x, y = truth.rows(rng, 5, n, dt("f64", cplx)), truth.rows(rng, 5, n, dt("f64", cplx))
            out = np.empty((5, 7), x.dtype)
            before = lib.fourier_emu_alloc_count()
            for b in (1, 5, 3):
                plan.correlate_ptr(x.ctypes.data, y.ctypes.data, out.ctypes.data, b)
                plan.correlate_ptr(x.ctypes.data, x.ctypes.data, out.ctypes.data, b)
            assert lib.fourier_emu_alloc_count() == before, (L, fusion)
            assert np.array_equal(run(plan, x, y), run(plan, x, y)), (L, fusion)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    lib = _lib.lib()
    fn = lambda op: getattr(lib, f"fourier_hip_xcorr_{op}_double")  # noqa: E731
    create, corr, status, opt, reserve = (fn(op) for op in ("create", "correlate", "last_status", "set_option", "reserve"))
    n = L = 16
    for bad in ((0, L, 0, L), (L + 1, L, 0, L), (n, L, 0, 0), (n, L, 0, L + 1), (n, L, L, 1), (n, L, -L, 1)):
        assert not create(*bad, 1, -1), bad
    assert not create(n, L, 0, L, 2, -1)
    plan = fa.CrossCorrelation(n, L, 0, L, "f64")
    h = plan._h
    assert (fn("size")(h), fn("length")(h), fn("lags")(h)) == (n, L, L)
    x, y, o = np.zeros((2, n)), np.zeros((2, n)), np.zeros((2, L))
    big = np.zeros(16 * x.size)
    X, Y, O, B = x.ctypes.data, y.ctypes.data, o.ctypes.data, big.ctypes.data
    row = 8 * n  # bytes of a row of reals (input and output rows alike here)
    assert corr(h, X, Y, O, 2, None) == 0 and status(h) == 0
    assert corr(h, None, Y, O, 2, None) == INVALID and status(h) == INVALID
    assert corr(h, X, None, O, 2, None) == INVALID and corr(h, X, Y, None, 2, None) == INVALID
    assert corr(h, X + 4, Y, O, 1, None) == INVALID and corr(h, X, Y + 4, O, 1, None) == INVALID  # reals: aligned to 8 bytes
    assert corr(h, X, Y, O + 4, 1, None) == INVALID
    assert corr(h, X + 8, Y + 8, O + 8, 1, None) == 0                # ... an odd real is enough
    assert corr(h, X, X, O, 2, None) == 0                            # x is y: the autocorrelation
    assert corr(h, B, Y, B, 2, None) == INVALID and corr(h, X, B, B, 2, None) == INVALID  # never in place
    assert corr(h, B + 2 * row, Y, B, 2, None) == 0                  # x behind the output: adjacent
    assert corr(h, B + 2 * row - 8, Y, B, 2, None) == INVALID        # ... one real earlier: inside it
    assert corr(h, X, B + 2 * row - 8, B, 2, None) == INVALID        # the same for y
    assert corr(h, B, Y, B + 2 * row, 2, None) == 0                  # the output behind x: adjacent
    assert corr(h, B, Y, B + 2 * row - 8, 2, None) == INVALID        # ... it begins inside x
    assert corr(h, X, B, B + 2 * row - 8, 2, None) == INVALID
    assert corr(h, X, Y, O, 0, None) == 0                            # batch 0: a no-op
    assert reserve(h, 0) == 0 and reserve(h, 2) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"weighting", 2) == INVALID and opt(h, b"weighting", -1) == INVALID
    assert opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"weighting", 1) == 0 and opt(h, b"fusion", 1) == 0 and plan.describe().startswith("xcorr composed")  # no kernel at L = 16
    # complex values: aligned to 2 * sizeof(T)
    cplan = fa.CrossCorrelation(n, L, 0, L, "f64", real_data=False)
    z = np.zeros((3, L), np.complex128)
    Z = z.ctypes.data
    assert corr(cplan._h, Z, Z, Z + 16 * L, 1, None) == 0
    assert corr(cplan._h, Z + 8, Z, Z + 16 * L, 1, None) == INVALID and corr(cplan._h, Z, Z, Z + 16 * L + 8, 1, None) == INVALID
    with pytest.raises(fa.FourierError):
        plan.correlate_ptr(0, Y, O, 1)
    with pytest.raises(fa.FourierError):
        plan.set_option("weighting", 7)
    for bad in ((0, 8, 0, 8), (9, 8, 0, 8), (8, 8, 0, 0), (8, 8, 0, 9), (8, 8, 8, 1), (8, 8, -8, 1)):
        with pytest.raises(ValueError):
            fa.CrossCorrelation(*bad)
    # the tensor layer refuses everything that is not a device tensor of the right dtype before it looks at shapes
    torch = pytest.importorskip("torch")
    for bad in (x, torch.zeros(2, n), torch.zeros(2, n, dtype=torch.complex64)):
        for call in (plan.correlate, fa.xcorr, fa.gcc_phat):
            with pytest.raises(TypeError):
                call(bad, bad)
    with pytest.raises(ValueError):
        fa.correlation_lags(8, 8)
    with pytest.raises(ValueError):
        fa.correlation_lags(8, 4, "circular")
    assert list(fa.correlation_lags(4)) == [-3, -2, -1, 0, 1, 2, 3] and list(fa.correlation_lags(4, 1)) == [-1, 0, 1]
    assert list(fa.correlation_lags(4, None, "circular")) == [0, 1, 2, 3] and list(fa.correlation_lags(5, 2, "circular")) == [-2, -1, 0, 1, 2]
