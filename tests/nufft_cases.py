"""The cases of the non-uniform FFT handle (fourier_hip_nufft_*, fourier_amd.Nufft) that tests/test_nufft_emu.py (CPU, the emulator
build) and its `-m gpu` twin tests/test_gpu_nufft.py both run, through Nufft.to_modes_ptr / to_points_ptr on raw buffers between
sentinel guard bands, against tests/nufft_truth.py (the direct sums in f64 on the inputs as rounded to the handle's type).  A test
module passes a backend: where the buffers live.

Strengths and modes are unit normal from fixed seeds, so no cancellation inflates the measure.

Measure and bound: relative L2 over the whole output of a call against the direct sum.
    w <= 6 (f32), w <= 12 (f64): the kernel error dominates:   3 x 10^(1 - w)
    above those widths:  3 x 10^(1 - w) + the rounding term, four times the error of the numpy model of the algorithm
                         (nufft_truth.Model) run in the handle's type on the same inputs
The numpy model in f64 measured err / 10^(1 - w) between 0.45 and 2.2 for w = 2 .. 14; every case first asserts, as a condition on
its inputs, that the f64 model itself is within 2.5 x 10^(1 - w) of the direct sum (for w <= 13; the only wider kernel tested is
w = 16, where the f64 model's own rounding, 4e-15 to 4e-14, is what it measures, and the figure is printed only).  Points that share
ONE cell add their kernel errors coherently: the sets "equal300", "last_cell" and "first_cell" give 3.1 to 4.5 x 10^(1 - w) in the f64
model at N = 100 (L = 2 N) and w = 13, so they are not valid inputs there and are placed at N = 101 (L = 216: 1.0 to 1.8);
sizes_for() says where each set runs.  A case prints ONE line with every figure of its
calls before it asserts them, each as t<type>:err/kernel term+rounding term(f64 model's error over 10^(1 - w)); the worst err / bound
per (precision, route, type) is printed at module end.

Shapes: the smallest at which the kernels can go wrong.  N = 1, 2, 3, 5 (2 w > 2 N sets L for the wider kernels), 100 (L = 2 N), 101
(L = 216 > 2 N), 500 (L = 1000, the smallest 2^a 3^b 5^c) and 512 (L = 1024, a power of two); the point sets of POINT_SETS; w at both
clamps, odd and even, through eps; batches 1, RB - 1, RB, RB + 1; both signs, both orders, both "table" routes."""
import re

import numpy as np
import pytest

import nufft_truth as truth
from convnd_cases import GUARD, INVALID, SENTINEL, DeviceBackend, HostBackend  # noqa: F401  (the backends are the same)
from helpers import rel_l2

RB = 4  # NUFFT_RB (fourier_amd/csrc/kernel_args.h)
BASE = {"f32": 2e-6, "f64": 1e-12}  # the project's single-transform figure
KERNEL_DOMINATES = {"f32": 6, "f64": 12}
MODEL_CHECKED = 13  # above it 2.5 x 10^(1 - w) is within reach of the f64 model's own rounding
EPS = {"f32": (0.5, 1e-3, 1e-6, 1e-9), "f64": (0.5, 1e-3, 1e-6, 1e-12, 1e-16)}  # w = 2, 4, 7, 8 and 2, 4, 7, 13, 16
TIGHT = {"f32": 1e-6, "f64": 1e-12}
SIZES = (1, 2, 3, 5, 100, 101, 500, 512)
POINT_SETS = ("empty", "at_zero", "at_minus_pi", "below_pi", "equal300", "last_cell", "first_cell", "ties", "far", "random37", "random3000")
ONE_CELL = ("equal300", "last_cell", "first_cell")
ROUTES = {0: "evaluated", 1: "tabulated"}
SCRATCH = "FOURIER_NUFFT_SCRATCH_BYTES"
LAUNCH = "FOURIER_LAUNCH_ITEMS"
WORST = {}
_MODELS = {}


def esize(real):
    return 4 if real == "f32" else 8


def crand(rng, shape, real):
    return np.ascontiguousarray((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(truth.cdt(real)))


def points(name, n, eps, real):
    """the point set `name` for a handle of n modes and accuracy eps (its grid length places the cell sets)"""
    rng = np.random.default_rng(len(name) * 131 + n)
    L = truth.grid_length(n, truth.width(eps, real))
    if name == "empty":
        return np.zeros(0)
    if name == "at_zero":
        return np.array([0.0])
    if name == "at_minus_pi":
        return np.array([-np.pi])
    if name == "below_pi":
        return np.array([np.nextafter(np.pi, 0.0)])
    if name == "equal300":
        return np.full(300, 1.2345)
    if name == "last_cell":  # grid coordinates in (L - 1, L): every footprint wraps over the top
        return 2 * np.pi * (L - 1 + rng.uniform(0.05, 0.95, 40)) / L
    if name == "first_cell":  # ... in (0, 1): every footprint begins below 0
        return 2 * np.pi * rng.uniform(0.05, 0.95, 40) / L
    if name == "ties":
        x = np.tile(rng.uniform(-np.pi, np.pi, 20), 3)
        rng.shuffle(x)
        return x
    if name == "far":
        return rng.uniform(-np.pi, np.pi, 37) + 2 * np.pi * rng.integers(-6, 7, 37)
    if name == "random37":
        return rng.uniform(-np.pi, np.pi, 37)
    if name == "random3000":
        return rng.uniform(-np.pi, np.pi, 3000)
    raise KeyError(name)


def sizes_for(name):
    """the N at which the point set `name` meets the condition on the inputs (the module docstring)"""
    return (101,) if name in ONE_CELL else (100, 101)


def models(n, eps, x, real):
    """the numpy model in f64 and in the handle's type for these points, computed once"""
    key = (n, eps, real, x.tobytes())
    if key not in _MODELS:
        _MODELS[key] = (truth.Model(n, eps, x, real), truth.Model(n, eps, x, real, real))
    return _MODELS[key]


def make(be, n, eps, real, table=0, **env):
    """a handle under the development switches `env` (read at create only), on the route of `table`"""
    for k, v in env.items():
        be.monkeypatch.setenv(k, str(v))
    try:
        plan = be.fa.Nufft(n, eps, real, be.device())
    finally:
        for k in env:
            be.monkeypatch.delenv(k)
    w = truth.width(eps, real)
    assert plan.modes() == n and plan.points() == 0
    assert plan.describe().startswith(f"nufft evaluated: w {w}, L {truth.grid_length(n, w)}, "), plan.describe()  # the default route
    plan.set_option("table", table)
    assert plan.describe().startswith(f"nufft {ROUTES[table]}: w {w}, L {truth.grid_length(n, w)}, "), plan.describe()
    return plan


def describe_numbers(plan):
    m = re.match(r"nufft \w+: w (\d+), L (\d+), ", plan.describe())
    return int(m.group(1)), int(m.group(2))


def set_points(be, plan, x):
    plan.set_points(np.asarray(x, np.float64))
    be.sync()
    assert plan.points() == len(x)


def run(be, plan, typ, v, sign, order=0):
    """type `typ` on v: (B, M) or (B, N), into a sentinel-filled buffer between guard bands; checks the bands and the input"""
    batch = v.shape[0]
    ovals = plan.modes() if typ == 1 else plan.points()
    count = batch * ovals
    vin = be.buf(v, GUARD, GUARD)
    out = be.buf(np.full(count, SENTINEL, v.dtype), GUARD, GUARD)
    before = vin.whole()
    (plan.to_modes_ptr if typ == 1 else plan.to_points_ptr)(vin.ptr, out.ptr, batch, sign, order)
    be.sync()
    after = out.whole()
    assert np.all(after[:GUARD] == SENTINEL) and np.all(after[GUARD + count:] == SENTINEL), "an element beside the output was written"
    assert vin.whole().tobytes() == before.tobytes(), "the call modified its input"
    return after[GUARD:GUARD + count].reshape(batch, ovals).copy()


def want_of(typ, x, v, n, sign, order):
    return truth.direct_modes(x, v, n, sign, order) if typ == 1 else truth.direct_points(x, v, sign, order)


def model_of(model, typ, v, sign, order):
    return model.to_modes(v, sign, order) if typ == 1 else model.to_points(v, sign, order)


def terms(real, n, eps, x, typ, v, sign, order, want):
    """(kernel term, rounding term, the f64 model's error over 10^(1 - w)) for this call; asserts the condition on the inputs"""
    w = truth.width(eps, real)
    m64, mt = models(n, eps, x, real)
    merr = rel_l2(model_of(m64, typ, v, sign, order), want) / 10.0 ** (1 - w)
    if w <= MODEL_CHECKED:
        assert merr <= 2.5, ("the inputs need more than the model gives", w, n, len(x), typ, merr)
    return 3 * 10.0 ** (1 - w), 4 * rel_l2(model_of(mt, typ, v, sign, order), want), merr


def bound(real, n, eps, x, typ, v, sign, order, want):
    """the bound of the module docstring for this call"""
    kernel, rounding, _ = terms(real, n, eps, x, typ, v, sign, order, want)
    return kernel + (rounding if truth.width(eps, real) > KERNEL_DOMINATES[real] else 0.0)


def note(be, real, table, what, figures):
    """figures: (type, err, (kernel term, rounding term, model figure)) of the calls of one case: ONE line with every figure as
    err/kernel+rounding(model), then the asserts"""
    w = int(re.search(r" w (\d+)", what).group(1))
    use = w > KERNEL_DOMINATES[real]
    print(f"nufft {be.where} {real} {ROUTES[table]} {what}: " + " ".join(f"t{typ}:{err:.3g}/{k:.3g}+{r:.3g}({m:.2g})" for typ, err, (k, r, m) in figures))
    for typ, err, (k, r, _) in figures:
        bnd = k + (r if use else 0.0)
        key = (real, ROUTES[table], typ)
        WORST[key] = max(WORST.get(key, 0.0), err / bnd)
        assert err <= bnd, (real, ROUTES[table], typ, what, err, bnd)


def report(where):
    for key, v in sorted(WORST.items()):
        print(f"nufft {where} worst err / bound {key}: {v:.3g}")


def accuracy(be, real, n, eps, x, table, batch=3, signs=(-1, 1), orders=(0, 1), what=""):
    """both types for every sign and order against the direct sums"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(7 * n + len(x) + batch)
    ins = {1: crand(rng, (batch, len(x)), real), 2: crand(rng, (batch, n), real)}
    figures = []
    for sign in signs:
        for order in orders:
            for typ in (1, 2):
                want = want_of(typ, x, ins[typ], n, sign, order)
                t = terms(real, n, eps, x, typ, ins[typ], sign, order, want)
                got = run(be, plan, typ, ins[typ], sign, order)
                if len(x) == 0 and typ == 1:
                    assert not got.any(), "no points: the modes are zeros"
                figures.append((typ, rel_l2(got, want), t))
    note(be, real, table, f"{what} n {n} m {len(x)} w {truth.width(eps, real)} batch {batch} signs {signs} orders {orders}", figures)
    return plan


# ---- structure
def adjoint(be, real, n, eps, x, table):
    """|<to_modes_s(c), f> - <c, to_points_{-s}(f)>| <= 4 base (||to_modes c|| ||f|| + ||c|| ||to_points f||), whatever eps is"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(41 + n)
    c, f = crand(rng, (1, len(x)), real), crand(rng, (1, n), real)
    gaps = []
    for sign in (-1, 1):
        for order in (0, 1):
            a = run(be, plan, 1, c, sign, order).astype(np.complex128)
            b = run(be, plan, 2, f, -sign, order).astype(np.complex128)
            c64, f64 = c.astype(np.complex128), f.astype(np.complex128)
            lhs, rhs = np.vdot(f64, a), np.vdot(b, c64)  # <a, f> = sum a conj(f); <c, b> = sum c conj(b)
            gap = abs(lhs - rhs)
            bnd = 4 * BASE[real] * (np.linalg.norm(a) * np.linalg.norm(f64) + np.linalg.norm(c64) * np.linalg.norm(b))
            gaps.append((gap, bnd))
    print(f"nufft {be.where} {real} {ROUTES[table]} adjoint n {n} m {len(x)} eps {eps} gap/bound: " + " ".join(f"{g:.3g}/{b:.3g}" for g, b in gaps))
    assert all(g <= b for g, b in gaps), (real, table, n, eps, gaps)


def routes_agree(be, real, n, eps, x):
    """the two "table" routes agree within twice the rounding term"""
    rng = np.random.default_rng(43 + n)
    ins = {1: crand(rng, (3, len(x)), real), 2: crand(rng, (3, n), real)}
    plans = [make(be, n, eps, real, table) for table in (0, 1)]
    for p in plans:
        set_points(be, p, x)
    for typ in (1, 2):
        want = want_of(typ, x, ins[typ], n, -1, 0)
        _, rounding, _ = terms(real, n, eps, x, typ, ins[typ], -1, 0, want)
        got = [run(be, p, typ, ins[typ], -1, 0) for p in plans]
        err = rel_l2(got[1], got[0])
        print(f"nufft {be.where} {real} routes type {typ} n {n} m {len(x)} eps {eps}: differ by {err:.3g}, twice the rounding term {2 * rounding:.3g}")
        assert err <= 2 * rounding, (real, typ, n, eps, err, rounding)


def orders_and_permutation(be, real, n, eps, table):
    """order 1 is ifftshift of order 0, bit for bit, in both directions; a permuted copy of the points (no ties) with the strengths
    permuted alike gives bit-equal modes; a repetition is bit-equal"""
    x = points("random37", n, eps, real)
    rng = np.random.default_rng(47 + n)
    c, f = crand(rng, (3, len(x)), real), crand(rng, (3, n), real)
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    for sign in (-1, 1):
        m0 = run(be, plan, 1, c, sign, 0)
        assert run(be, plan, 1, c, sign, 0).tobytes() == m0.tobytes(), "a repetition differs"
        assert run(be, plan, 1, c, sign, 1).tobytes() == np.fft.ifftshift(m0, axes=-1).tobytes(), "order 1 is not ifftshift of order 0"
        p0 = run(be, plan, 2, f, sign, 0)
        assert run(be, plan, 2, f, sign, 0).tobytes() == p0.tobytes(), "a repetition differs"
        assert run(be, plan, 2, np.ascontiguousarray(np.fft.ifftshift(f, axes=-1)), sign, 1).tobytes() == p0.tobytes()
    perm = rng.permutation(len(x))
    other = make(be, n, eps, real, table)
    set_points(be, other, x[perm])
    m0 = run(be, plan, 1, c, -1, 0)
    assert run(be, other, 1, np.ascontiguousarray(c[:, perm]), -1, 0).tobytes() == m0.tobytes(), "permuted points give other bits"
    p0 = run(be, plan, 2, f, 1, 0)
    assert run(be, other, 2, f, 1, 0).tobytes() == np.ascontiguousarray(p0[:, perm]).tobytes()


def walk(be, real, n, eps, x, table, batch, **env):
    """both types of a handle under the development switches `env` and of one without: the pairs of results, checked against the truth"""
    rng = np.random.default_rng(53 + batch)
    ins = {1: crand(rng, (batch, len(x)), real), 2: crand(rng, (batch, n), real)}
    w = truth.width(eps, real)
    res = {}
    for e in (env, {}):
        plan = make(be, n, eps, real, table, **e)
        set_points(be, plan, x)
        for typ in (1, 2):
            res.setdefault(typ, []).append(run(be, plan, typ, ins[typ], -1, 0))
    figures = []
    for typ in (1, 2):
        want = want_of(typ, x, ins[typ], n, -1, 0)
        figures.append((typ, rel_l2(res[typ][0], want), terms(real, n, eps, x, typ, ins[typ], -1, 0, want)))
    note(be, real, table, f"n {n} m {len(x)} w {w} batch {batch} under {env}", figures)
    return res


def launch_walk(be, real, n, eps, x, table, batch, items):
    """FOURIER_LAUNCH_ITEMS splits the four new kernels' launches; the transforms' calls are the same, so every bit is"""
    res = walk(be, real, n, eps, x, table, batch, **{LAUNCH: items})
    for typ in (1, 2):
        assert res[typ][0].tobytes() == res[typ][1].tobytes(), (real, n, table, batch, items, typ, "differs from the unbounded handle")


def scratch_walk(be, real, n, eps, x, table, rows):
    """batch 5 under a scratch bound of `rows` fine-grid rows: bit for bit the unbounded handle's result at f64, and at f32 under the
    bound of two rows; under one row f32 holds the bound only (the f32 inner row kernels' last bits depend on a row's parity within
    its launch)"""
    L = truth.grid_length(n, truth.width(eps, real))
    res = walk(be, real, n, eps, x, table, 5, **{SCRATCH: rows * L * 2 * esize(real)})
    if real == "f64" or rows % 2 == 0:
        for typ in (1, 2):
            assert res[typ][0].tobytes() == res[typ][1].tobytes(), (real, n, table, rows, typ, "differs from the unbounded handle")


def nan_row(be, real, n, eps, x, table):
    """a NaN strength (or mode) in one row leaves every other row bit-equal; run() checks the guard bands"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(59)
    for typ, vals in ((1, len(x)), (2, n)):
        v = crand(rng, (RB + 1, vals), real)
        clean = run(be, plan, typ, v, -1, 0)
        bad = v.copy()
        bad[2, vals // 2] = np.nan
        got = run(be, plan, typ, bad, -1, 0)
        assert np.isnan(got[2]).any()
        keep = [0, 1, 3, 4]
        assert got[keep].tobytes() == clean[keep].tobytes(), (real, table, typ, "a NaN in row 2 changed another row")


def second_set_points_replaces(be, real, table):
    n, eps = 100, TIGHT[real]
    plan = make(be, n, eps, real, table)
    rng = np.random.default_rng(61)
    for name in ("random3000", "random37", "ties"):  # fewer points after more: nothing of the first set is left
        x = points(name, n, eps, real)
        set_points(be, plan, x)
        c = crand(rng, (2, len(x)), real)
        want = truth.direct_modes(x, c, n, -1)
        note(be, real, table, f"set_points again: {name} w {truth.width(eps, real)}", [(1, rel_l2(run(be, plan, 1, c, -1, 0), want), terms(real, n, eps, x, 1, c, -1, 0, want))])


def refusals(be, real):
    """refused with INVALID and no write: a call before set_points, a NaN point (the points stay), overlapping buffers, an unknown
    option, a sign of 0, an order of 2"""
    n, eps = 16, 1e-3
    fa = be.fa
    plan = make(be, n, eps, real)
    x = points("random37", n, eps, real)
    rng = np.random.default_rng(67)
    c = crand(rng, (2, len(x)), real)
    cin = be.buf(c, 0, 64)
    out = be.buf(np.full(2 * max(n, len(x)), SENTINEL, c.dtype))
    untouched = out.whole().tobytes()
    e = 2 * esize(real)

    def refused(call, *args):
        with pytest.raises(fa.FourierError):
            call(*args)
        be.sync()
        assert out.whole().tobytes() == untouched, "a refused call wrote"

    refused(plan.to_modes_ptr, cin.ptr, out.ptr, 2, -1, 0)   # before any set_points
    refused(plan.to_points_ptr, cin.ptr, out.ptr, 2, 1, 0)
    set_points(be, plan, x)
    good = run(be, plan, 1, c, -1, 0)
    bad = x.copy()
    bad[5] = np.nan
    with pytest.raises(ValueError):
        plan.set_points(bad)                                 # the Python layer refuses it ...
    for v in (np.nan, np.inf):
        bad[5] = v
        with pytest.raises(fa.FourierError):
            plan.set_points_ptr(bad.ctypes.data, len(bad))   # ... and so does the library
    assert plan.points() == len(x) and run(be, plan, 1, c, -1, 0).tobytes() == good.tobytes(), "a refused set_points changed the points"
    for sign, order in ((0, 0), (2, 0), (-1, 2), (1, -1)):
        refused(plan.to_modes_ptr, cin.ptr, out.ptr, 2, sign, order)
        refused(plan.to_points_ptr, cin.ptr, out.ptr, 2, sign, order)
    refused(plan.to_modes_ptr, 0, out.ptr, 2, -1, 0)          # null
    refused(plan.to_modes_ptr, cin.ptr, 0, 2, -1, 0)
    refused(plan.to_modes_ptr, cin.ptr + e // 2, out.ptr, 2, -1, 0)  # aligned to one real only
    refused(plan.to_modes_ptr, out.ptr, out.ptr, 2, -1, 0)    # in place
    refused(plan.to_modes_ptr, out.ptr + e, out.ptr, 2, -1, 0)  # overlapping
    refused(plan.to_points_ptr, out.ptr, out.ptr + e, 2, 1, 0)
    for key, v in (("table", 2), ("table", -1), ("fusion", 1), ("no_such_option", 0)):
        with pytest.raises(fa.FourierError):
            plan.set_option(key, v)
    plan.to_modes_ptr(cin.ptr, out.ptr, 0, -1, 0)             # batch 0: a no-op
    be.sync()
    assert out.whole().tobytes() == untouched
    assert run(be, plan, 1, c, -1, 0).tobytes() == good.tobytes()
