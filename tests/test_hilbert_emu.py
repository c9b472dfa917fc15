"""The analytic-signal handle (fourier_hip_hilbert_*, fourier_amd.Hilbert) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against tests/hilbert_truth.py (f64 numpy on
the rounded input).  The `-m gpu` twin is tests/test_gpu_hilbert.py, which also holds the argument checks that need device tensors (the
last dimension, `N` padding and truncation, a non-last `dim`).

Inputs: seeded white Gaussian rows.  Tolerance, relative L2 over the whole output: 2 x base, base the single-transform figure
tests/test_gpu_real.py grants the route -- f32 2e-6 (4e-6 on a Bluestein plan), f64 1e-13 (1e-11 on a Bluestein plan) -- because two
transforms in T contribute (the rule by which tests/test_gpu_conv.py takes 3 x).  The envelope has the same bound: ||z'| - |z|| <=
|z' - z| and || |z| || = ||z||.  Every figure is printed before it is asserted; the worst of a run, as a fraction of its bound, is
printed at the end."""
import ctypes

import numpy as np
import pytest

import hilbert_truth as truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, output, route) -> the largest err / bound seen
COMPOSED_ONLY = (1, 2, 3, 7, 16, 64, 100, 255, 1000, 1001, 1031)
FUSED = (2048, 4096, 16384, 32768)


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
        print(f"hilbert emu worst err / bound {key}: {v:.3g}")


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return 2 * base


def has_fused(real, n):
    return n in (2048, 4096, 8192, 16384) or (n == 32768 and real == "f32")


def route_of(plan):
    return "one-launch" if plan.describe().startswith("hilbert one-launch") else "composed"


def run(plan, x, what, first=1):
    """analytic_ptr / envelope_ptr into a buffer whose output starts on element `first` (1: an odd element) with sentinels on both sides;
    checks them and that the input is unmodified"""
    batch, n = x.shape
    bx = x.tobytes()
    count = batch * n
    buf = np.full(count + first + 2, SENTINEL, cdt(plan.real) if what == "analytic" else rdt(plan.real))
    out = buf[first:first + count]
    getattr(plan, what + "_ptr")(x.ctypes.data, out.ctypes.data, batch)
    assert np.all(buf[:first] == SENTINEL) and np.all(buf[-2:] == SENTINEL), "an element beside the output was written"
    assert x.tobytes() == bx, f"{what} modified its input"
    return out.reshape(batch, n).copy()


def note(real, what, route, err, bound, n):
    print(f"{what} {real} N={n} {route}: err {err:.3g} bound {bound:.3g}")
    key = (real, what, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, (real, what, route, n, err, bound)


def check(fa, real, n, batch):
    """both "fusion" values with the describe string asserted; the analytic signal and the envelope against the truth, Re z = x, the
    upper half of fft(z) empty, and the two routes within 2 x the tolerance of each other"""
    rng = np.random.default_rng(1000 * batch + n)
    x = truth.rows(rng, batch, n, rdt(real))
    want = truth.analytic(x)
    spectrum = np.linalg.norm(np.fft.fft(x.astype(np.float64), axis=-1))
    plan = fa.Hilbert(n, real)
    assert plan.size() == n
    assert plan.describe().startswith("hilbert composed"), plan.describe()  # the default route
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        route = "one-launch" if fusion and has_fused(real, n) else "composed"
        assert plan.describe().startswith(f"hilbert {route}: "), plan.describe()
        bound = tol(plan, real)
        z, env = run(plan, x, "analytic"), run(plan, x, "envelope")
        note(real, "analytic", route, rel_l2(z, want), bound, n)
        note(real, "envelope", route, rel_l2(env, np.abs(want)), bound, n)
        note(real, "real part", route, rel_l2(z.real, x), bound, n)
        if n >= 4:
            upper = np.linalg.norm(np.fft.fft(z.astype(np.complex128), axis=-1)[:, n // 2 + 1:])
            note(real, "upper half", route, upper / spectrum, bound, n)
        got[route] = z, env, bound
    if len(got) == 2:
        bound = 2 * max(got["one-launch"][2], got["composed"][2])
        for i, what in enumerate(("analytic", "envelope")):
            note(real, what, "routes", rel_l2(got["one-launch"][i], got["composed"][i]), bound, n)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("n", COMPOSED_ONLY)
def test_composed_sizes(fa, real, n):
    for batch in (3, 5):
        check(fa, real, n, batch)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("n", FUSED)
def test_fused_sizes_on_both_routes(fa, real, n):
    if n == 32768 and real == "f64":  # no f64 kernel of that length: "fusion" = 1 stays on the composed route
        plan = fa.Hilbert(n, real)
        plan.set_option("fusion", 1)
        assert plan.describe().startswith("hilbert composed"), plan.describe()
        return
    for batch in (3, 5):
        check(fa, real, n, batch)


@pytest.mark.parametrize("fusion", [1, 0])
def test_f32_envelope_on_bases_that_are_only_4_byte_aligned(fa, fusion):
    """the element-wise load and store of the one-launch kernel (and the composed route on the same pointers): bit-equal to the
    aligned call"""
    n, batch = 2048, 3
    rng = np.random.default_rng(5)
    x = truth.rows(rng, batch, n, np.float32)
    holder = np.zeros(batch * n + 1, np.float32)
    shifted = holder[1:].reshape(batch, n)
    shifted[...] = x
    assert x.ctypes.data % 8 == 0 and shifted.ctypes.data % 8 == 4
    plan = fa.Hilbert(n, "f32")
    plan.set_option("fusion", fusion)
    aligned = run(plan, x, "envelope", first=2)
    odd = run(plan, shifted, "envelope", first=1)
    assert np.array_equal(aligned, odd)
    note("f32", "envelope", route_of(plan) + " unaligned", rel_l2(odd, truth.envelope(x)), tol(plan, "f32"), n)
    # ... and the analytic signal from an input that is only 4-byte aligned
    assert np.array_equal(run(plan, x, "analytic"), run(plan, shifted, "analytic"))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_envelope_in_place(fa, real):
    rng = np.random.default_rng(6)
    for n in (100, 255, 2048):
        x = truth.rows(rng, 5, n, rdt(real))
        plan = fa.Hilbert(n, real)
        for fusion in (1, 0):
            plan.set_option("fusion", fusion)
            want = run(plan, x, "envelope")
            y = x.copy()
            plan.envelope_ptr(y.ctypes.data, y.ctypes.data, 5)
            assert np.array_equal(y, want), (real, n, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(fa, real, monkeypatch):
    rng = np.random.default_rng(7)
    elem = 8 if real == "f32" else 16
    for n in (100, 255, 2048):
        x = truth.rows(rng, 5, n, rdt(real))
        whole = fa.Hilbert(n, real)
        per = (n // 2 + 1 + n) * elem  # the half spectrum and the envelope's analytic signal of one row
        monkeypatch.setenv("FOURIER_HILBERT_SCRATCH_BYTES", str(2 * per + 8))  # two rows a chunk: 5 rows in 3 chunks
        small = fa.Hilbert(n, real)
        monkeypatch.delenv("FOURIER_HILBERT_SCRATCH_BYTES")
        for plan in (whole, small):
            assert plan.describe().startswith("hilbert composed")
        for what in ("analytic", "envelope"):
            a, b = run(whole, x, what), run(small, x, what)
            assert np.array_equal(a, b), (real, n, what)
            want = truth.analytic(x)
            note(real, what, "composed chunks", rel_l2(b, want if what == "analytic" else np.abs(want)), tol(small, real), n)


def test_reserve_then_calls_do_not_allocate_and_repeat_bit_equal(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(8)
    for n in (1000, 2048):
        for fusion in (1, 0):
            plan = fa.Hilbert(n, "f64")
            plan.set_option("fusion", fusion)
            plan.reserve(5)
            x = truth.rows(rng, 5, n, np.float64)
            z, e = np.empty((5, n), np.complex128), np.empty((5, n))
            before = L.fourier_emu_alloc_count()
            for b in (1, 5, 3):
                plan.analytic_ptr(x.ctypes.data, z.ctypes.data, b)
                plan.envelope_ptr(x.ctypes.data, e.ctypes.data, b)
            assert L.fourier_emu_alloc_count() == before, (n, fusion)
            first = run(plan, x, "analytic"), run(plan, x, "envelope")
            again = run(plan, x, "analytic"), run(plan, x, "envelope")
            assert all(np.array_equal(a, b) for a, b in zip(first, again)), (n, fusion)


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    fn = lambda op: getattr(L, f"fourier_hip_hilbert_{op}_double")  # noqa: E731
    create, ana, env, status, opt, reserve = (fn(op) for op in ("create", "analytic", "envelope", "last_status", "set_option", "reserve"))
    assert not create(0, -1)
    n = 16
    plan = fa.Hilbert(n, "f64")
    h = plan._h
    assert fn("size")(h) == n
    x = np.zeros((2, n))
    z = np.zeros((2, n), np.complex128)
    e = np.zeros((2, n))
    big = np.zeros(16 * x.size)
    X, Z, E, B = x.ctypes.data, z.ctypes.data, e.ctypes.data, big.ctypes.data
    row = 8 * n  # bytes of a row of reals
    assert ana(h, X, Z, 2, None) == 0 and status(h) == 0
    assert ana(h, None, Z, 2, None) == INVALID and status(h) == INVALID
    assert ana(h, X, None, 2, None) == INVALID
    assert ana(h, X + 4, Z, 1, None) == INVALID              # reals: aligned to 8 bytes
    assert ana(h, X, Z + 8, 1, None) == INVALID              # complex values: aligned to 16
    assert ana(h, X + 8, Z, 1, None) == 0                    # ... an odd real is enough for the input
    assert ana(h, B, B, 2, None) == INVALID                  # never in place: the output is twice the input
    assert ana(h, B + 2 * row, B, 1, None) == 0              # the input behind the output: adjacent
    assert ana(h, B + 2 * row - 8, B, 1, None) == INVALID    # ... one real earlier: inside it
    assert ana(h, B, B + 2 * row, 2, None) == 0              # the output behind the input: adjacent
    assert ana(h, B, B + 2 * row - 16, 2, None) == INVALID   # ... it begins inside the input
    assert ana(h, X, Z, 0, None) == 0                        # batch 0: a no-op
    assert env(h, X, E, 2, None) == 0 and status(h) == 0
    assert env(h, None, E, 2, None) == INVALID and status(h) == INVALID
    assert env(h, X, None, 2, None) == INVALID
    assert env(h, X + 4, E, 1, None) == INVALID
    assert env(h, X, E + 4, 1, None) == INVALID
    assert env(h, X, E + 8, 1, None) == 0                    # reals out: aligned to 8
    assert env(h, B, B, 2, None) == 0                        # in place
    assert env(h, B, B + 8, 2, None) == INVALID              # any other overlap
    assert env(h, B + row, B, 2, None) == INVALID
    assert env(h, B, B + 2 * row, 2, None) == 0              # adjacent
    assert env(h, X, E, 0, None) == 0
    assert reserve(h, 0) == 0 and reserve(h, 2) == 0
    assert opt(h, b"fusion", 2) == INVALID and opt(h, b"no_such_option", 1) == INVALID and opt(h, None, 1) == INVALID
    assert opt(h, b"fusion", 1) == 0 and plan.describe().startswith("hilbert composed")  # no one-launch kernel at N = 16
    with pytest.raises(fa.FourierError):
        plan.analytic_ptr(0, Z, 1)
    with pytest.raises(fa.FourierError):
        plan.envelope_ptr(X, 0, 1)
    with pytest.raises(ValueError):
        fa.Hilbert(0, "f32")
    # the tensor layer refuses everything that is not a device tensor of a real dtype before it looks at shapes
    torch = pytest.importorskip("torch")
    for bad in (x, torch.zeros(2, n), torch.zeros(2, n, dtype=torch.complex64)):
        for call in (plan.analytic, plan.envelope, fa.hilbert, fa.envelope):
            with pytest.raises(TypeError):
                call(bad)
