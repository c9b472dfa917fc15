"""The cases of the cepstrum handle (fourier_hip_cepstrum_*, fourier_amd.Cepstrum) that tests/test_cepstrum_emu.py (CPU, the emulator
build) and its `-m gpu` twin tests/test_gpu_cepstrum.py both run, through Cepstrum.apply_ptr on raw buffers, against
tests/cepstrum_truth.py (f64 numpy on the inputs as rounded to the handle's type).  A test module passes a backend: where the buffers
live.

Inputs: batches of 6 rows, each x[0] = 1 plus 0.2 N(0, 1) / sqrt(n) on every sample, from a fixed seed.  With the X of the truth,
kappa = ||x||_2 / min_k max(|X_k|, log_floor).  Every case asserts the CONDITIONS kappa <= 4 and max |Im C_k| <= pi, so that a badly
conditioned draw cannot hide behind the bound.

Measure and bound, per row, the worst row of a call:
    CEPSTRUM       err = ||got - want||_2 / (|log_mult| kappa)                   bound 3 x base (forward, log and untangle, inverse);
                   rigorous to first order from ||dX||_2 <= base ||X||_2 (tests/cepstrum_truth.py)
    MINIMUM_PHASE  err = ||got - want||_2 / (||h_full||_2 |log_mult| kappa)      bound 6 x base; h_full the truth's whole row of L
base is the single-transform figure of tests/test_gpu_real.py: f32 2e-6, f64 1e-13, and 4e-6 / 1e-11 where describe() names a
Bluestein plan.  An f32 numpy model of both chains gives 0.5 - 1.1e-7 (cepstrum) and 1.0 - 2.0e-7 (minimum phase) at every shape
here.  Every figure is printed before it is asserted; the worst err / bound per (precision, mode, route) is printed at module end."""
import numpy as np

import cepstrum_truth as truth

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, mode, route) -> the largest err / bound seen
DEFAULT_FUSION = 1  # the handle's default of "fusion" (cepstrum_plan.h; DESIGN.md section 4, "Cepstrum and minimum phase")
MODES = (truth.CEPSTRUM, truth.MINIMUM_PHASE)
MODE_NAME = {truth.CEPSTRUM: "real cepstrum", truth.MINIMUM_PHASE: "minimum phase"}

# (L, n, m): all of n; odd n and m, so the unpaired f32 load and store; m < n; m = L > n; the largest length of the precision
ONE_LAUNCH = {"f32": ((2048, 2048, 2048), (2048, 1501, 1501), (2048, 1024, 300), (4096, 2049, 4096), (32768, 20000, 20000)),
              "f64": ((2048, 2048, 2048), (2048, 1501, 1501), (2048, 1024, 300), (4096, 2049, 4096), (16384, 10000, 10000))}
COMPOSED = (7, 16, 255, 1000, 1031, 2048)
# The one-launch instances that the product holds (kernels_cepstrum.cpp): (precision, mode) -> lengths.  The f32 minimum-phase
# kernels of 2^13 and 2^15 spill more than the envelope kernel of their shape and exist in the experiments library and the emulator
# build only, behind the development switch FOURIER_CEPSTRUM_SPILLING (read at create): a test that runs them passes spilling=True.
KERNELS = {("f32", 0): (2048, 4096, 8192, 16384, 32768), ("f32", 1): (2048, 4096, 16384),
           ("f64", 0): (2048, 4096, 8192, 16384), ("f64", 1): (2048, 4096, 8192, 16384)}
SPILLING = "FOURIER_CEPSTRUM_SPILLING"


def ndt(real):
    return np.float32 if real == "f32" else np.float64


def has_kernel(real, mode, L):
    return L in KERNELS[real, mode]


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def bound(plan, real, mode):
    return (3 if mode == truth.CEPSTRUM else 6) * base(plan, real)


class HostBackend:
    """buffers in host memory: the emulator build"""

    def __init__(self, fa):
        self.fa = fa

    class Buf:
        def __init__(self, values, before=0, after=0):
            values = np.ascontiguousarray(values)
            self.hold = np.full(values.size + before + after, SENTINEL, values.dtype)
            self.view = self.hold[before:before + values.size]
            self.view[...] = values.ravel()
            self.ptr = self.view.ctypes.data

        def whole(self):
            return self.hold.copy()

    def buf(self, values, before=0, after=0):
        return self.Buf(values, before, after)

    def sync(self):
        pass


class DeviceBackend:
    """buffers in device memory (torch tensors)"""

    def __init__(self, fa, torch):
        self.fa, self.torch = fa, torch

    def buf(self, values, before=0, after=0):
        torch = self.torch
        values = np.ascontiguousarray(values)

        class Buf:
            pass

        b = Buf()
        b.hold = torch.full((values.size + before + after,), SENTINEL, dtype=torch.from_numpy(values[:0].ravel()).dtype, device="cuda")
        b.hold[before:before + values.size] = torch.from_numpy(values.ravel()).cuda()
        b.ptr = b.hold.data_ptr() + before * values.dtype.itemsize
        b.whole = lambda: b.hold.cpu().numpy()
        return b

    def sync(self):
        self.torch.cuda.synchronize()


def make(be, n, L, m, real, mode, fusion=0, spilling=False):
    plan = be.fa.Cepstrum(n, L, real, m, mode, *((0,) if isinstance(be, DeviceBackend) else ()))
    assert (plan.size(), plan.length(), plan.outputs(), plan.mode()) == (n, L, m, mode)
    fused = has_kernel(real, mode, L) or (spilling and has_kernel(real, 0, L))
    default = "one-launch" if fused and DEFAULT_FUSION else "composed"
    assert plan.describe().startswith(f"cepstrum {default} ({MODE_NAME[mode]}): "), plan.describe()
    plan.set_option("fusion", fusion)
    route = "one-launch" if fusion and fused else "composed"
    assert plan.describe().startswith(f"cepstrum {route} ({MODE_NAME[mode]}): "), plan.describe()
    return plan, route


GUARD = 4  # sentinels behind every buffer


def run(be, plan, x, log_mult=1.0, log_floor=0.0, first=1, in_first=0, in_place=False):
    """apply_ptr into a buffer whose output starts on element `first` (1: an odd element) with sentinel guard bands on both sides, from
    an input that starts on element `in_first` between guard bands of its own; checks the bands and that the input is unmodified
    (in_place: the output IS the input)"""
    batch, n = x.shape
    m = plan.outputs()
    xin = be.buf(x, in_first, GUARD)
    out = xin if in_place else be.buf(np.zeros(batch * m, x.dtype), first, GUARD)
    off = in_first if in_place else first
    before = xin.whole()
    plan.apply_ptr(xin.ptr, out.ptr, batch, log_mult, log_floor)
    be.sync()
    after = out.whole()
    assert np.all(after[:off] == SENTINEL) and np.all(after[-GUARD:] == SENTINEL), "an element beside the output was written"
    if not in_place:
        assert xin.whole().tobytes() == before.tobytes(), "apply modified its input"
    return after[off:off + batch * m].reshape(batch, m).copy()


def note(real, mode, route, what, err, bnd):
    print(f"cepstrum {real} {MODE_NAME[mode]} {route} {what}: err {err:.3g} bound {bnd:.3g} ratio {err / bnd:.3g}")
    key = (real, MODE_NAME[mode], route)
    WORST[key] = max(WORST.get(key, 0.0), err / bnd)
    assert err <= bnd, (real, mode, route, what, err, bnd)


def report(where):
    for key, v in sorted(WORST.items()):
        print(f"cepstrum {where} worst err / bound {key}: {v:.3g}")


def conditions(x, L, log_mult=1.0, log_floor=0.0):
    """the conditions under which the bounds are claimed; printed, then asserted"""
    k = float(truth.kappa(x, L, log_floor).max())
    ph = truth.max_phase(x, L, log_mult, log_floor)
    print(f"cepstrum conditions L={L} n={x.shape[1]}: kappa {k:.3g} max |Im C| {ph:.3g}")
    assert k <= 4 and ph <= np.pi, (L, x.shape, k, ph)


def check(be, plan, real, mode, route, x, L, what, log_mult=1.0, log_floor=0.0, **kw):
    out = run(be, plan, x, log_mult, log_floor, **kw)
    note(real, mode, route, what, truth.err(mode, out, x, L, plan.outputs(), log_mult, log_floor), bound(plan, real, mode))
    return out


# ---- one launch: against the truth, aligned and unaligned bases, repetition, in place
def one_launch(be, real, mode, L, n, m, spilling=False):
    rng = np.random.default_rng(L + n + m)
    x = truth.rows(rng, 6, n, ndt(real))
    conditions(x, L)
    plan, route = make(be, n, L, m, real, mode, 1, spilling)
    assert route == "one-launch"
    got = {}
    # output on an even element from an input on element 0 (f32: both 8-byte aligned, the `pairs` path where n, m are even), then
    # both on an odd element: the base is offset by one T, and the `pairs` path is not taken
    for first, in_first in ((2, 0), (1, 1)):
        got[first] = check(be, plan, real, mode, route, x, L, f"L={L} n={n} m={m} bases=({in_first}, {first})", first=first, in_first=in_first)
        assert np.array_equal(run(be, plan, x, first=first, in_first=in_first), got[first]), (real, mode, L, n, "repetition differs")
        if m == n:
            inp = run(be, plan, x, in_first=in_first, in_place=True)
            assert np.array_equal(inp, got[first]), (real, mode, L, n, "in place differs")
    assert np.array_equal(got[2], got[1]), (real, mode, L, n, "the unaligned call differs from the aligned one")


# ---- composed: every kind of length; n < L and n == L; m == L on an aligned base (the direct store) and m < L (the window sweep)
def composed(be, real, mode, L):
    for n in sorted({L, max(1, (3 * L + 2) // 5)}):
        rng = np.random.default_rng(100 * L + n)
        x = truth.rows(rng, 6, n, ndt(real))
        conditions(x, L)
        for m, first in ((L, 2), (L, 1), (max(1, (2 * L) // 3), 1)):
            plan, route = make(be, n, L, m, real, mode, 0)
            assert route == "composed"
            out = check(be, plan, real, mode, route, x, L, f"L={L} n={n} m={m} first={first}", first=first)
            assert np.array_equal(run(be, plan, x, first=first), out), (real, mode, L, n, m, "repetition differs")
            if m == n:
                for in_first in (0, 1):
                    assert np.array_equal(run(be, plan, x, in_first=in_first, in_place=True), out), (real, mode, L, n, "in place differs")


# ---- the two routes agree within the sum of their bounds
def routes_agree(be, real, mode, L, n):
    rng = np.random.default_rng(7 * L + n)
    x = truth.rows(rng, 6, n, ndt(real))
    conditions(x, L)
    out = {}
    bnd = 0.0
    for fusion in (1, 0):
        plan, route = make(be, n, L, n, real, mode, fusion)
        assert route == ("one-launch" if fusion else "composed")
        out[route] = run(be, plan, x)
        bnd += bound(plan, real, mode)
    want = truth.full(mode, x, L)
    den = truth.kappa(x, L) * (np.linalg.norm(want, axis=-1) if mode == truth.MINIMUM_PHASE else 1.0)
    diff = float(np.max(np.linalg.norm(out["one-launch"].astype(np.float64) - out["composed"], axis=-1) / den))
    note(real, mode, "routes", f"L={L} n={n}", diff, bnd)


# ---- known answers
def known_answers(be, real, fusion):
    """x = [1, -a]: c[0] = 0, c[q] = -a^q / (2 q); minimum_phase([-a, 1]) = [1, -a]; minimum_phase([1, -a]) = [1, -a]"""
    L, a, b = 2048, 0.5, base_of(real)
    x = np.zeros((6, 64), ndt(real))
    x[:, 0], x[:, 1] = 1.0, -a
    plan, route = make(be, 64, L, 40, real, truth.CEPSTRUM, fusion)
    c = run(be, plan, x)
    q = np.arange(1, 40)
    want = np.concatenate(([0.0], -a ** q / (2 * q)))
    worst = float(np.abs(c - want).max())
    note(real, truth.CEPSTRUM, route, "c[q] = -a^q / (2 q)", worst, 3 * b)
    for name, row in (("maximum phase [-a, 1]", (-a, 1.0)), ("minimum phase [1, -a]", (1.0, -a))):
        x[:, 0], x[:, 1] = row
        plan, route = make(be, 64, L, 64, real, truth.MINIMUM_PHASE, fusion)
        h = run(be, plan, x)
        want = np.zeros(64)
        want[0], want[1] = 1.0, -a
        den = np.linalg.norm(want) * float(truth.kappa(x, L).max())
        note(real, truth.MINIMUM_PHASE, route, name, float(np.linalg.norm(h - want, axis=-1).max() / den), 6 * b)


def base_of(real):
    return 2e-6 if real == "f32" else 1e-13


def magnitude_is_kept(be, real, fusion):
    """random rows, m = L: |fft(h)| equals |X| within 6 x base x kappa relative to ||X||"""
    L, n = 2048, 1501
    rng = np.random.default_rng(17)
    x = truth.rows(rng, 6, n, ndt(real))
    conditions(x, L)
    plan, route = make(be, n, L, L, real, truth.MINIMUM_PHASE, fusion)
    h = run(be, plan, x)
    X = np.abs(truth.spectrum(x, L))
    H = np.abs(np.fft.fft(h.astype(np.float64), axis=-1))
    rel = np.linalg.norm(H - X, axis=-1) / np.linalg.norm(X, axis=-1) / truth.kappa(x, L)
    note(real, truth.MINIMUM_PHASE, route, "|fft(h)| = |X|", float(rel.max()), 6 * base(plan, real))


# ---- the floor
def floor_on_a_zero_row(be, real, fusion):
    """an all-zero row with log_floor = 1e-3: c = [log_mult ln(1e-3), 0, ...] within 3 x base x |c[0]|, h = [1e-3^log_mult, 0, ...]"""
    L, n = (2048, 1501) if fusion else (1000, 600)
    x = np.zeros((6, n), ndt(real))
    for mode in MODES:
        for log_mult in (1.0, 0.5):
            plan, route = make(be, n, L, n, real, mode, fusion)
            out = run(be, plan, x, log_mult, 1e-3)
            want = np.zeros(n)
            fl = float(ndt(real)(1e-3))
            want[0] = log_mult * np.log(fl) if mode == truth.CEPSTRUM else fl ** log_mult
            rel = float(np.linalg.norm(out - want, axis=-1).max() / abs(want[0]))
            note(real, mode, route, f"zero rows, log_floor=1e-3 log_mult={log_mult}", rel, bound(plan, real, mode))


FLOORS = {"f32": (1e-18, 1e-19, 1e-25, 1e-37, 1e30, 1e38), "f64": (1e-150, 1e-200, 1e-300, 1e200, 1e300)}


def floor_whose_square_leaves_the_format(be, real, fusion):
    """Every positive floor that is a normal number of T is honoured, whatever log_floor^2 does in T (FLOORS: the first of each
    precision has a normal square, the small ones after it a square that is subnormal or 0, the large ones a square that is inf).
    Six rows, rows 1 and 4 zero, both modes, log_mult 1 and 0.5:
      the zero rows are [log_mult ln floor, 0, ...] (minimum phase [floor^log_mult, 0, ...]) under floor_on_a_zero_row's bound;
      under a floor whose square is below the smallest normal number the other rows are BIT-equal to the call with log_floor = 0;
      under a floor whose square is inf every row is the zero row's, under the same bound.
    Before the handle took the value of a floored bin from the host for such a floor: f32 1e-25 gave -inf / NaN in the zero rows (one-launch
    [-inf, nan, ...], composed all NaN), 1e30 gave [inf, nan, ...] / NaN in every row; f64 1e-200 and 1e200 the same."""
    L, n = (2048, 1501) if fusion else (1000, 600)
    dt = ndt(real)
    x = truth.rows(np.random.default_rng(29), 6, n, dt)
    zero, other = [1, 4], [0, 2, 3, 5]
    x[zero] = 0
    worst, failed = {}, []
    for mode in MODES:
        plan, route = make(be, n, L, n, real, mode, fusion)
        for log_mult in (1.0, 0.5):
            free = run(be, plan, x, log_mult, 0.0)
            for floor in FLOORS[real]:
                fl = float(dt(floor))
                with np.errstate(over="ignore", under="ignore"):
                    square = float(dt(fl) * dt(fl))
                out = run(be, plan, x, log_mult, floor).astype(np.float64)
                want = np.zeros(n)
                want[0] = log_mult * np.log(fl) if mode == truth.CEPSTRUM else fl ** log_mult
                rows = zero if np.isfinite(square) else [0, 1, 2, 3, 4, 5]
                with np.errstate(invalid="ignore"):
                    rel = float(np.linalg.norm((out[rows] - want) / abs(want[0]), axis=-1).max())  # (the quotient first: 1e300^2 overflows)
                rel = rel if rel == rel else np.inf
                bnd = bound(plan, real, mode)
                key = (MODE_NAME[mode], log_mult)
                if rel / bnd >= worst.get(key, (0.0,))[0]:
                    worst[key] = (rel / bnd, rel, bnd, floor)
                if not rel <= bnd:
                    failed.append((MODE_NAME[mode], log_mult, floor, "floored rows", rel, bnd, out[rows[0], :3].tolist()))
                if square < np.finfo(dt).tiny and not np.array_equal(out[other].astype(dt), free[other]):
                    failed.append((MODE_NAME[mode], log_mult, floor, "a row above the floor differs from the call without a floor"))
    for (name, log_mult), (ratio, rel, bnd, floor) in sorted(worst.items()):
        print(f"cepstrum {real} {name} {route} floors {FLOORS[real]} log_mult={log_mult}: worst err {rel:.3g} bound {bnd:.3g} ratio {ratio:.3g} (log_floor={floor:g})")
        key = (real, name, route)
        if ratio == ratio and ratio != np.inf:
            WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert not failed, (real, route, failed)


def zero_floor_on_a_zero_row(be, real, mode, fusion):
    """the same row with log_floor = 0, as row 3 of 6: rows 0 - 2 and 4 - 5 are bit-equal to a call without it, row 3 is not finite,
    and nothing outside the output is touched (run checks the guard bands)"""
    L, n = (2048, 1501) if fusion else (1000, 600)
    rng = np.random.default_rng(19)
    x = truth.rows(rng, 6, n, ndt(real))
    plan, route = make(be, n, L, n, real, mode, fusion)
    clean = run(be, plan, x)
    x[3] = 0
    out = run(be, plan, x)
    assert not np.any(np.isfinite(out[3])), (real, mode, route, "finite values in the row of a zero spectrum")
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(out[keep], clean[keep]), (real, mode, route, "another row changed")


# ---- log_mult
def log_mult_half(be, real, mode, fusion):
    L, n = (2048, 1501) if fusion else (1000, 600)
    rng = np.random.default_rng(23)
    x = truth.rows(rng, 6, n, ndt(real))
    conditions(x, L, 0.5)
    plan, route = make(be, n, L, n, real, mode, fusion)
    check(be, plan, real, mode, route, x, L, f"L={L} n={n} log_mult=0.5", 0.5)
    conditions(x, L, -1.0, 0.7)
    check(be, plan, real, mode, route, x, L, f"L={L} n={n} log_mult=-1 log_floor=0.7", -1.0, 0.7)


# ---- chunk and launch walks (development switches: the emulator build and the experiments library read them at create)
def row_bytes(real, L):
    """the scratch of one row on the composed route (cepstrum_plan.h)"""
    rs = 4 if real == "f32" else 8
    return (L // 2 + 1) * 2 * rs + 2 * L * rs


def walks(be, monkeypatch, real, mode):
    """6 rows.  FOURIER_CEPSTRUM_SCRATCH_BYTES of two rows: chunks of an EVEN number of rows, every row keeps its parity within its
    launch -> bit-equal to the unbounded handle at f64 and at f32.  FOURIER_CEPSTRUM_SCRATCH_BYTES of one row and FOURIER_LAUNCH_BYTES
    of one row: chunks / launches of exactly ONE row -> bit-equal at f64; at f32 the odd rows lose their parity, the known deviation of
    the inner transforms (section 4, "Cross-correlation"), so the result is asserted within the bound only.
    FOURIER_LAUNCH_ITEMS = 4 on the one-launch route: launches of 4 and 2 rows -> bit-equal."""
    rs = 4 if real == "f32" else 8
    cases = []  # (switch, value, L, n, fusion, parity kept)
    for L, n in ((1000, 600), (2048, 1501)):
        cases.append(("FOURIER_CEPSTRUM_SCRATCH_BYTES", 2 * row_bytes(real, L) + 8, L, n, 0, True))
        cases.append(("FOURIER_CEPSTRUM_SCRATCH_BYTES", row_bytes(real, L) + 8, L, n, 0, False))
        cases.append(("FOURIER_LAUNCH_BYTES", (L // 2 + 1) * 2 * rs + 8, L, n, 0, False))
    cases.append(("FOURIER_LAUNCH_ITEMS", 4, 2048, 1501, 1, True))
    rng = np.random.default_rng(13)
    for switch, value, L, n, fusion, parity in cases:
        x = truth.rows(rng, 6, n, ndt(real))
        whole, _ = make(be, n, L, n, real, mode, fusion)
        monkeypatch.setenv(switch, str(value))
        try:
            bounded, route = make(be, n, L, n, real, mode, fusion)
        finally:
            monkeypatch.delenv(switch)
        a, b = run(be, whole, x), run(be, bounded, x)
        equal = np.array_equal(a, b)
        print(f"cepstrum {real} {MODE_NAME[mode]} {switch}={value} L={L}: bit-equal {equal}, max diff {np.abs(a - b).max():.3g}")
        note(real, mode, route, f"{switch}={value} L={L}", truth.err(mode, b, x, L, n), bound(bounded, real, mode))
        if real == "f64" or parity:
            assert equal, (real, mode, switch, L)
