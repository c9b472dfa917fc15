"""The chirp-z handle (fourier_hip_czt_*, fourier_amd.Czt) WITHOUT a GPU: the engine sources compiled against the CPU emulation
(tests/emu), driven through the same C ABI / Python layer as the product, on the cases of tests/czt_cases.py (shapes, parameter sets,
tolerance: base x R, base f32 4e-6 / f64 1e-11) against tests/czt_truth.py (the exact-phase direct sum in f64 on the rounded input).
The `-m gpu` twin is tests/test_gpu_czt.py, which adds the batch of 1025 rows, graph replay and the torch layer.

A numpy model with tables and intermediates rounded to T gives 1.3e-7 ... 1.6e-7 (f32) and 7e-16 ... 9e-16 (f64) on these parameter
sets; the emulator runs the true kernels' arithmetic, so it shows that they stay inside the bound before any GPU run.  Every figure is
printed before it is asserted; the worst of a run, as a fraction of its bound, is printed at the end."""
import ctypes

import numpy as np
import pytest

import czt_cases as cases
import czt_truth as truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
WORST = {}


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
        print(f"czt emu worst err / bound {key}: {v:.3g}")


class Backend:
    device = -1

    @staticmethod
    def run(plan, x, first=1):
        batch = x.shape[0]
        bx = x.tobytes()
        count = batch * plan.points()
        buf = np.full(count + first + 2, cases.SENTINEL, cases.cdt(plan.real))
        out = buf[first:first + count]
        plan.transform_ptr(x.ctypes.data, out.ctypes.data, batch)
        assert np.all(buf[:first] == cases.SENTINEL) and np.all(buf[-2:] == cases.SENTINEL), "an element beside the output was written"
        assert x.tobytes() == bx, "transform modified its input"
        return out.reshape(batch, plan.points()).copy()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("L", [2048, 4096])
def test_one_launch_shapes_on_both_routes(fa, real, L):
    for n, m in cases.one_launch_shapes(L):
        cases.check(Backend, fa, real, n, m, worst=WORST)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_largest_one_launch_length_without_slack(fa, real):
    L = cases.TOP[real]
    cases.check(Backend, fa, real, L // 2, L // 2 + 1, worst=WORST)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("L", [2048, 4096])
def test_real_input(fa, real, L):
    for n, m in cases.real_shapes(L):
        cases.check(Backend, fa, real, n, m, real_input=True, worst=WORST)


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("n", [1800, 1031])
def test_f32_real_input_offset_by_one_real(fa, fusion, n):
    """the scalar loads (an input that is only 4-byte aligned; n odd) against the paired ones: bit-equal to the aligned call"""
    m, batch = {1800: 249, 1031: 999}[n], 5
    x = truth.rows(np.random.default_rng(5), batch, n, np.float32)
    holder = np.zeros(batch * n + 1, np.float32)
    shifted = holder[1:].reshape(batch, n)
    shifted[...] = x
    assert x.ctypes.data % 8 == 0 and shifted.ctypes.data % 8 == 4
    plan = fa.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, "f32", True)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith("czt one-launch" if fusion else "czt composed")
    aligned, odd = Backend.run(plan, x), Backend.run(plan, shifted)
    assert np.array_equal(aligned, odd)
    cases.note(WORST, "f32", "zoom real offset", "one-launch" if fusion else "composed", (n, m),
               rel_l2(odd, truth.czt(x, m, 1.0, -0.1 / m, 1.0, 0.2)), cases.BASE["f32"])


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(fa, real):
    for n, m in ((1, 1), (3, 5), (255, 1000)):
        res = cases.check(Backend, fa, real, n, m, worst=WORST)
        assert res
    for n, m in ((1, 1), (3, 5)):  # a tiny plan has no convolution route: forward, product, inverse
        plan = fa.Czt(n, m, real=real)
        assert plan.describe().startswith("czt composed: forward, product, inverse: "), plan.describe()  # L < 2048: the default


def test_f32_fused_pass_convolution_at_2_to_the_16(fa):
    res = cases.check(Backend, fa, "f32", 20000, 20000, batch=3, sets=("zoom",), worst=WORST, routes=(1,))
    assert set(res) == {("zoom", "composed")}  # "fusion" = 1 has no one-launch kernel at L = 2^16
    plan = fa.Czt(20000, 20000, real="f32")
    assert plan.describe().startswith("czt composed: conv fused passes: "), plan.describe()


def test_f64_above_its_largest_kernel_stays_composed(fa):
    plan = fa.Czt(10000, 10000, real="f64")  # L = 2^15: f32 has a one-launch kernel, f64 has none
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("czt composed: "), plan.describe()
    plan = fa.Czt(10000, 10000, real="f32")
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("czt one-launch: "), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_dft_identity_at_65536(fa, real):
    """n = m = 65536, w_turns = -2^-16 (exact), a = 1: the whole output against np.fft.fft in f64 -- an unreduced or half-index chirp,
    which a 1000-point case cannot show, is far outside the bound here"""
    n = 65536
    x = truth.rows(np.random.default_rng(16), 1, n, cases.cdt(real))
    plan = fa.Czt(n, n, 1.0, -(2.0 ** -16), 1.0, 0.0, real)
    out = Backend.run(plan, x)
    cases.note(WORST, real, "dft identity", "composed", (n, n), rel_l2(out, np.fft.fft(x.astype(np.complex128), axis=-1)), cases.BASE[real])


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(fa, real, monkeypatch):
    n, m, L = 255, 1000, 2048
    x = truth.rows(np.random.default_rng(7), 5, n, cases.cdt(real))
    whole = fa.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, real)
    per = L * (8 if real == "f32" else 16)  # the work row
    monkeypatch.setenv("FOURIER_CZT_SCRATCH_BYTES", str(2 * per + 8))  # two rows a chunk: 5 rows in 3 chunks
    small = fa.Czt(n, m, 1.0, -0.1 / m, 1.0, 0.2, real)
    monkeypatch.delenv("FOURIER_CZT_SCRATCH_BYTES")
    for plan in (whole, small):
        plan.set_option("fusion", 0)
        assert plan.describe().startswith("czt composed")
    a, b = Backend.run(whole, x), Backend.run(small, x)
    assert np.array_equal(a, b)
    cases.note(WORST, real, "zoom", "composed chunks", (n, m), rel_l2(b, truth.czt(x, m, 1.0, -0.1 / m, 1.0, 0.2)), cases.BASE[real])


def test_reserve_then_calls_do_not_allocate_and_repeat_bit_equal(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for n, m in ((3, 5), (255, 1000), (700, 300)):
        for fusion in (1, 0):
            plan = fa.Czt(n, m, real="f64")
            plan.set_option("fusion", fusion)
            plan.reserve(5)
            x = truth.rows(rng, 5, n, np.complex128)
            z = np.empty((5, m), np.complex128)
            before = L.fourier_emu_alloc_count()
            for b in (1, 5, 3):
                plan.transform_ptr(x.ctypes.data, z.ctypes.data, b)
            assert L.fourier_emu_alloc_count() == before, (n, m, fusion)
            assert np.array_equal(Backend.run(plan, x), Backend.run(plan, x)), (n, m, fusion)


def test_create_refuses_what_the_tables_cannot_carry(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    for s in ("float", "double"):
        create = getattr(L, f"fourier_hip_czt_create_{s}")
        assert not create(0, 4, 1.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(4, 0, 1.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(4, 4, 0.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(4, 4, -1.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(4, 4, 1.0, -0.25, 0.0, 0.0, 0, -1)
        for i in range(4):
            for bad in (float("nan"), float("inf")):
                pars = [1.0, -0.25, 1.0, 0.0]
                pars[i] = bad
                assert not create(4, 4, *pars, 0, -1)
        assert not create((1 << 26) + 1, 1, 1.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(1 << 25, (1 << 25) + 2, 1.0, -0.25, 1.0, 0.0, 0, -1)
        assert not create(100, 100, 2.0, -0.01, 1.0, 0.0, 0, -1)  # w_abs^(99^2 / 2) = 2^4900: a spiral no T carries
    assert not L.fourier_hip_czt_create_float(100, 100, 1.05, -0.01, 1.0, 0.0, 0, -1)  # 1.05^4900 = 1e104: f64 carries it, f32 does not
    h = L.fourier_hip_czt_create_double(100, 100, 1.05, -0.01, 1.0, 0.0, 0, -1)
    assert h
    L.fourier_hip_czt_destroy_double(h)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_czt_{op}_double")  # noqa: E731
    tr, status, opt, reserve = (fn(op) for op in ("transform", "last_status", "set_option", "reserve"))
    n, m = 16, 8
    plan = fa.Czt(n, m, real="f64")
    h = plan._h
    assert fn("size")(h) == n and fn("points")(h) == m
    x = np.zeros((2, n), np.complex128)
    z = np.zeros((2, m), np.complex128)
    big = np.zeros(64 * n, np.complex128)
    X, Z, B = x.ctypes.data, z.ctypes.data, big.ctypes.data
    irow, orow = 16 * n, 16 * m
    assert tr(h, X, Z, 2, None) == 0 and status(h) == 0
    assert tr(h, None, Z, 2, None) == INVALID and status(h) == INVALID
    assert tr(h, X, None, 2, None) == INVALID
    assert tr(h, X + 8, Z, 1, None) == INVALID                 # complex values: aligned to 16 bytes
    assert tr(h, X, Z + 8, 1, None) == INVALID
    assert tr(h, X + 16, Z, 1, None) == 0                      # ... an odd element is enough
    assert tr(h, B, B, 2, None) == INVALID                     # never in place
    assert tr(h, B + 2 * orow, B, 2, None) == 0                # the input behind the output: adjacent
    assert tr(h, B + 2 * orow - 16, B, 2, None) == INVALID     # ... one element earlier: inside it
    assert tr(h, B, B + 2 * irow, 2, None) == 0                # the output behind the input: adjacent
    assert tr(h, B, B + 2 * irow - 16, 2, None) == INVALID     # ... it begins inside the input
    assert tr(h, X, Z, 0, None) == 0 and status(h) == 0        # batch 0: a no-op
    assert reserve(h, 0) == 0 and reserve(h, 2) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("czt one-launch")  # L = max(2048, 32)
    # real input rows: aligned to one real
    rplan = fa.Czt(n, m, real="f64", real_input=True)
    r = np.zeros((2, n + 1))
    R = r.ctypes.data
    rt = lambda *a: fn("transform")(rplan._h, *a)  # noqa: E731
    assert rt(R, Z, 2, None) == 0 and rt(R + 8, Z, 2, None) == 0 and rt(R + 4, Z, 2, None) == INVALID
    with pytest.raises(fa.FourierError):
        plan.transform_ptr(0, Z, 1)
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            fa.Czt(*bad)
    for kw in ({"w_abs": 0.0}, {"a_abs": -1.0}, {"w_turns": float("nan")}, {"a_turns": float("inf")}):
        with pytest.raises(ValueError):
            fa.Czt(4, 4, **kw)
    # the tensor layer refuses everything that is not a device tensor of the handle's dtype before it looks at shapes
    torch = pytest.importorskip("torch")
    for bad in (x, torch.zeros(2, n, dtype=torch.complex128), torch.zeros(2, n, dtype=torch.float64)):
        with pytest.raises(TypeError):
            plan.transform(bad)
    for bad in (x, torch.zeros(2, n), torch.zeros(2, n, dtype=torch.complex64)):
        for call in (lambda t: fa.czt(t), lambda t: fa.zoom_fft(t, 0.5)):
            with pytest.raises(TypeError):
                call(bad)


def test_truth_vectorised_phases_match_exact_integer_arithmetic():
    """czt_truth.phases against czt_truth.exact_phases (Python ints, one rounding): within the 3.5e-16 of a turn its docstring derives"""
    for n, m, w_turns, a_turns in ((1024, 1025, -0.1 / 1025, 0.2), (300, 200, -1 / 200, 0.0), (2000, 64, -0.1 / 20000, 0.2), (50, 60, 0.37, -5.3),
                                   (40, 30, -(2.0 ** -16), 0.0), (30, 40, 1e-300, 0.1)):
        bins = range(m) if m != 64 else [int(k) for k in cases.sample_bins(20000)]
        d = truth.phases(n, bins, w_turns, a_turns) - truth.exact_phases(n, bins, w_turns, a_turns)
        d -= np.round(d)
        print(f"phases n={n} m={m} w_turns={w_turns} a_turns={a_turns}: max difference {np.abs(d).max():.3g} turns")
        assert np.abs(d).max() <= 3.5e-16


def test_scipy_agrees_where_its_own_error_allows():
    """scipy.signal.czt is NOT the truth (its w**(k**2/2) is 2e-12 off at n = 100); a cross-check of the definition at 1e-9"""
    signal = pytest.importorskip("scipy.signal")
    x = truth.rows(np.random.default_rng(3), 2, 100, np.complex128)
    w, a = 0.999 * np.exp(-2j * np.pi * 0.003), 1.01 * np.exp(2j * np.pi * 0.2)
    want = signal.czt(x, 50, w, a, axis=-1)
    got = truth.czt(x, 50, abs(w), np.angle(w) / (2 * np.pi), abs(a), np.angle(a) / (2 * np.pi))
    assert rel_l2(got, want) <= 1e-9
