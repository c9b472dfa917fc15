"""The cases of the 3-D non-uniform FFT handle (fourier_hip_nufft3d_*, fourier_amd.Nufft3d) that tests/test_nufft3d_emu.py (CPU, the
emulator build) and its `-m gpu` twin tests/test_gpu_nufft3d.py both run, through Nufft3d.to_modes_ptr / to_points_ptr on raw buffers
between sentinel guard bands, against tests/nufft3d_truth.py (the direct sums in f64 on the inputs as rounded to the handle's type).
A test module passes a backend: where the buffers live.  Every run asserts that the call did not modify its input.

Strengths and modes are unit normal from fixed seeds, so no cancellation inflates the measure.

Measure and bound: relative L2 over the whole output of a call against the direct sum.
    w <= 6 (f32), w <= 12 (f64): the kernel error dominates:   9 x 10^(1 - w), the 1-D figure of 3 once per axis (2-D uses 6)
    above those widths:  9 x 10^(1 - w) + the rounding term, four times the error of the numpy model of the algorithm
                         (nufft3d_truth.Model) run in the handle's type on the same inputs
Every case first asserts, as a condition on its inputs, that the f64 model itself is within 7.5 x 10^(1 - w) of the direct sum (for
w <= 13; the only wider kernel tested is w = 16, where the f64 model's own rounding is what it measures, and the figure is printed
only).  Points that share ONE cell add their kernel errors coherently: the single-cell sets "equal300" and "at_corner" are not run at
(2, 3, 4) and (30, 4, 9), where an independent f64 model gave 5.4 - 5.5 at w = 4; test_point_sets runs every set at (8, 9, 10) and
(20, 6, 21), "random3000" at (8, 9, 10) and (16, 16, 16); sizes_for() says so.  Over every call of these cases (both types, both
signs, w = 2 .. 13) the committed f64 model measured at most 4.0, at "equal300" on (20, 6, 21) with w = 7 (f32), and at most 2.8
everywhere else: no set nears the condition, so none was moved.  The largest figure of a run is printed at module end.  A case
prints ONE line with every figure of its calls before it asserts them, each as
t<type>:err/kernel term+rounding term(f64 model's error over 10^(1 - w)); the worst err / bound per (precision, route, type) is
printed at module end.

Shapes: the smallest at which the kernels can go wrong, as (n1, n2, n3); the grid is L1 x L2 x L3, axis 3 its rows.  (1, 1, 1):
L = 2 w on every axis, all wraps; (2, 3, 4); (3, 40, 5), where 2 w > 2 n sets L on axes 1 and 3; (8, 9, 10): f32 grid 16 x 18 x 20,
f64 grid 27^3, every length odd; (20, 6, 21): f32 40 x 15 x 45, one even length and odd rows; (30, 4, 9): f32 60 x 15 x 18, two even
lengths; (16, 16, 16): 32^3, a power-of-two grid.  The point sets of POINT_SETS; w at both clamps, odd and even, through eps;
batches 1, RB - 1, RB, RB + 1, 2 RB + 1; both signs, both orders, both "table" routes."""
import re

import numpy as np
import pytest

import nufft3d_truth as truth
from convnd_cases import GUARD, INVALID, SENTINEL, DeviceBackend, HostBackend  # noqa: F401  (the backends are the same)
from helpers import rel_l2
from nufft_cases import BASE, EPS, KERNEL_DOMINATES, MODEL_CHECKED, RB, ROUTES, TIGHT, crand, esize  # noqa: F401  (the 1-D handle's)

KERNEL_TERM = 9.0     # x 10^(1 - w)
MODEL_WITHIN = 7.5    # x 10^(1 - w): the condition on the inputs
SIZES = ((1, 1, 1), (2, 3, 4), (3, 40, 5), (8, 9, 10), (20, 6, 21), (30, 4, 9), (16, 16, 16))
POINT_SETS = ("empty", "at_zero", "at_corner", "equal300", "corner_cell", "wrap1", "wrap2", "wrap3", "ties", "far", "random37", "random3000")
SCRATCH = "FOURIER_NUFFT3D_SCRATCH_BYTES"
LAUNCH = "FOURIER_LAUNCH_ITEMS"
WORST = {}
MODEL_WORST = [0.0]   # the largest f64-model figure (w <= MODEL_CHECKED) of the calls of this run, printed at module end
_MODELS = {}


def grid(n, eps, real):
    w = truth.width(eps, real)
    return tuple(truth.grid_length(n[d], w) for d in range(3))


def points(name, n, eps, real):
    """the point set `name` as (x1, x2, x3) for a handle of n = (n1, n2, n3) modes and accuracy eps (its grid lengths place the cell sets)"""
    rng = np.random.default_rng(len(name) * 131 + 49 * n[0] + 7 * n[1] + n[2])
    L = grid(n, eps, real)
    two_pi = 2 * np.pi

    def last_cell(L, k):  # grid coordinates in (L - 1, L): every footprint wraps over the top
        return two_pi * (L - 1 + rng.uniform(0.05, 0.95, k)) / L

    def first_cell(L, k):  # ... in (0, 1): every footprint begins below 0
        return two_pi * rng.uniform(0.05, 0.95, k) / L

    def inside(k):  # between 0.26 and 0.74 of the period: no footprint wraps (L >= 2 w)
        return two_pi * rng.uniform(0.26, 0.74, k)

    def uniform(k):
        return tuple(rng.uniform(-np.pi, np.pi, k) for _ in range(3))

    if name == "empty":
        return np.zeros(0), np.zeros(0), np.zeros(0)
    if name == "at_zero":
        return np.array([0.0]), np.array([0.0]), np.array([0.0])
    if name == "at_corner":
        return np.array([-np.pi]), np.array([np.nextafter(np.pi, 0.0)]), np.array([np.pi])
    if name == "equal300":
        return np.full(300, 1.2345), np.full(300, -2.3456), np.full(300, 0.3456)
    if name == "corner_cell":  # the last cell of axes 1 and 3 and the first of axis 2: every footprint wraps on all three axes
        return last_cell(L[0], 40), first_cell(L[1], 40), last_cell(L[2], 40)
    if name in ("wrap1", "wrap2", "wrap3"):
        d = int(name[-1]) - 1
        x = [inside(40), inside(40), inside(40)]
        x[d] = np.concatenate([last_cell(L[d], 20), first_cell(L[d], 20)])
        return tuple(x)
    if name == "ties":
        x = np.tile(rng.uniform(-np.pi, np.pi, (20, 3)), (3, 1))
        rng.shuffle(x, axis=0)
        return x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy()
    if name == "far":
        return tuple(v + two_pi * rng.integers(-6, 7, 37) for v in uniform(37))
    if name == "random37":
        return uniform(37)
    if name == "random3000":
        return uniform(3000)
    raise KeyError(name)


def sizes_for(name):
    """the sizes at which the point set `name` runs in test_point_sets (every one meets the condition on the inputs there)"""
    return ((8, 9, 10), (16, 16, 16)) if name == "random3000" else ((8, 9, 10), (20, 6, 21))


def models(n, eps, x, real):
    """the numpy model in f64 and in the handle's type for these points, computed once"""
    key = (n, eps, real) + tuple(v.tobytes() for v in x)
    if key not in _MODELS:
        _MODELS[key] = (truth.Model(n, eps, x[0], x[1], x[2], real), truth.Model(n, eps, x[0], x[1], x[2], real, real))
    return _MODELS[key]


def prefix(route, n, eps, real):
    L1, L2, L3 = grid(n, eps, real)
    return f"nufft3d {route}: w {truth.width(eps, real)}, L {L1} x {L2} x {L3}, "


def make(be, n, eps, real, table=0, **env):
    """a handle under the development switches `env` (read at create only), on the route of `table`"""
    for k, v in env.items():
        be.monkeypatch.setenv(k, str(v))
    try:
        plan = be.fa.Nufft3d(n, eps, real, be.device())
    finally:
        for k in env:
            be.monkeypatch.delenv(k)
    assert plan.modes() == tuple(n) and plan.points() == 0
    assert plan.describe().startswith(prefix("evaluated", n, eps, real)), plan.describe()  # the default route
    plan.set_option("table", table)
    assert plan.describe().startswith(prefix(ROUTES[table], n, eps, real)), plan.describe()
    return plan


def describe_numbers(plan):
    m = re.match(r"nufft3d \w+: w (\d+), L (\d+) x (\d+) x (\d+), rows .*, axis 2 .*, axis 1 ", plan.describe())
    return tuple(int(m.group(i)) for i in range(1, 5))


def set_points(be, plan, x):
    plan.set_points(*(np.asarray(v, np.float64) for v in x))
    be.sync()
    assert plan.points() == len(x[0])


def run(be, plan, typ, v, sign, order=0):
    """type `typ` on v: (B, M) or (B, n1, n2, n3), into a sentinel-filled buffer between guard bands; checks the bands and the input"""
    batch = v.shape[0]
    oshape = (batch,) + plan.modes() if typ == 1 else (batch, plan.points())
    count = int(np.prod(oshape))
    vin = be.buf(v, GUARD, GUARD)
    out = be.buf(np.full(count, SENTINEL, v.dtype), GUARD, GUARD)
    before = vin.whole()
    (plan.to_modes_ptr if typ == 1 else plan.to_points_ptr)(vin.ptr, out.ptr, batch, sign, order)
    be.sync()
    after = out.whole()
    assert np.all(after[:GUARD] == SENTINEL) and np.all(after[GUARD + count:] == SENTINEL), "an element beside the output was written"
    assert vin.whole().tobytes() == before.tobytes(), "the call modified its input"
    return after[GUARD:GUARD + count].reshape(oshape).copy()


def inputs(rng, batch, n, m, real):
    return {1: crand(rng, (batch, m), real), 2: crand(rng, (batch,) + tuple(n), real)}


def want_of(typ, x, v, n, sign, order):
    return truth.direct_modes(x[0], x[1], x[2], v, n, sign, order) if typ == 1 else truth.direct_points(x[0], x[1], x[2], v, sign, order)


def model_of(model, typ, v, sign, order):
    return model.to_modes(v, sign, order) if typ == 1 else model.to_points(v, sign, order)


def terms(real, n, eps, x, typ, v, sign, order, want):
    """(kernel term, rounding term, the f64 model's error over 10^(1 - w)) for this call; asserts the condition on the inputs"""
    w = truth.width(eps, real)
    m64, mt = models(n, eps, x, real)
    merr = rel_l2(model_of(m64, typ, v, sign, order), want) / 10.0 ** (1 - w) if want.size else 0.0
    if w <= MODEL_CHECKED:
        MODEL_WORST[0] = max(MODEL_WORST[0], merr)
        assert merr <= MODEL_WITHIN, ("the inputs need more than the model gives", w, n, len(x[0]), typ, merr)
    rounding = 4 * rel_l2(model_of(mt, typ, v, sign, order), want) if want.size else 0.0
    return KERNEL_TERM * 10.0 ** (1 - w), rounding, merr


def bound(real, n, eps, x, typ, v, sign, order, want):
    """the bound of the module docstring for this call"""
    kernel, rounding, _ = terms(real, n, eps, x, typ, v, sign, order, want)
    return kernel + (rounding if truth.width(eps, real) > KERNEL_DOMINATES[real] else 0.0)


def err_of(got, want):
    return rel_l2(got, want) if want.size else 0.0


def note(be, real, table, what, figures):
    """figures: (type, err, (kernel term, rounding term, model figure)) of the calls of one case: ONE line with every figure as
    err/kernel+rounding(model), then the asserts"""
    w = int(re.search(r" w (\d+)", what).group(1))
    use = w > KERNEL_DOMINATES[real]
    print(f"nufft3d {be.where} {real} {ROUTES[table]} {what}: " + " ".join(f"t{typ}:{err:.3g}/{k:.3g}+{r:.3g}({m:.2g})" for typ, err, (k, r, m) in figures))
    for typ, err, (k, r, _) in figures:
        bnd = k + (r if use else 0.0)
        key = (real, ROUTES[table], typ)
        WORST[key] = max(WORST.get(key, 0.0), err / bnd)
        assert err <= bnd, (real, ROUTES[table], typ, what, err, bnd)


def report(where):
    for key, v in sorted(WORST.items()):
        print(f"nufft3d {where} worst err / bound {key}: {v:.3g}")
    print(f"nufft3d {where} worst f64 model figure (w <= {MODEL_CHECKED}): {MODEL_WORST[0]:.3g} x 10^(1 - w), condition {MODEL_WITHIN}")


def accuracy(be, real, n, eps, x, table, batch=3, signs=(-1, 1), orders=(0, 1), what=""):
    """both types for every sign and order against the direct sums"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    m = len(x[0])
    rng = np.random.default_rng(49 * n[0] + 7 * n[1] + n[2] + m + batch)
    ins = inputs(rng, batch, n, m, real)
    figures = []
    for sign in signs:
        for order in orders:
            for typ in (1, 2):
                want = want_of(typ, x, ins[typ], n, sign, order)
                t = terms(real, n, eps, x, typ, ins[typ], sign, order, want)
                got = run(be, plan, typ, ins[typ], sign, order)
                if m == 0 and typ == 1:
                    assert not got.any(), "no points: the modes are zeros"
                figures.append((typ, err_of(got, want), t))
    note(be, real, table, f"{what} n {n} m {m} w {truth.width(eps, real)} batch {batch} signs {signs} orders {orders}", figures)
    return plan


# ---- structure
def adjoint(be, real, n, eps, x, table):
    """|<to_modes_s(c), f> - <c, to_points_{-s}(f)>| <= 12 base (||to_modes c|| ||f|| + ||c|| ||to_points f||), whatever eps is: the
    1-D factor 4 times the three transforms per item"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(41 + n[0] + n[1] + n[2])
    ins = inputs(rng, 1, n, len(x[0]), real)
    c, f = ins[1], ins[2]
    gaps = []
    for sign in (-1, 1):
        for order in (0, 1):
            a = run(be, plan, 1, c, sign, order).astype(np.complex128)
            b = run(be, plan, 2, f, -sign, order).astype(np.complex128)
            c64, f64 = c.astype(np.complex128), f.astype(np.complex128)
            lhs, rhs = np.vdot(f64, a), np.vdot(b, c64)  # <a, f> = sum a conj(f); <c, b> = sum c conj(b)
            gap = abs(lhs - rhs)
            bnd = 12 * BASE[real] * (np.linalg.norm(a) * np.linalg.norm(f64) + np.linalg.norm(c64) * np.linalg.norm(b))
            gaps.append((gap, bnd))
    print(f"nufft3d {be.where} {real} {ROUTES[table]} adjoint n {n} m {len(x[0])} eps {eps} gap/bound: " + " ".join(f"{g / b:.3g}" for g, b in gaps))
    assert all(g <= b for g, b in gaps), (real, table, n, eps, gaps)


def routes_agree(be, real, n, eps, x):
    """the two "table" routes agree within twice the rounding term"""
    rng = np.random.default_rng(43 + n[0] + n[1] + n[2])
    ins = inputs(rng, 3, n, len(x[0]), real)
    plans = [make(be, n, eps, real, table) for table in (0, 1)]
    for p in plans:
        set_points(be, p, x)
    for typ in (1, 2):
        want = want_of(typ, x, ins[typ], n, -1, 0)
        _, rounding, _ = terms(real, n, eps, x, typ, ins[typ], -1, 0, want)
        got = [run(be, p, typ, ins[typ], -1, 0) for p in plans]
        err = rel_l2(got[1], got[0])
        print(f"nufft3d {be.where} {real} routes type {typ} n {n} m {len(x[0])} eps {eps}: differ by {err:.3g}, twice the rounding term {2 * rounding:.3g}")
        assert err <= 2 * rounding, (real, typ, n, eps, err, rounding)


def shift3(v):
    return np.ascontiguousarray(np.fft.ifftshift(v, axes=(-3, -2, -1)))


def orders_and_permutation(be, real, n, eps, table):
    """order 1 is ifftshift over the three axes of order 0, bit for bit, in both directions; a permuted copy of the points (no two
    share a third coordinate) with the strengths permuted alike gives bit-equal modes and the permuted values; a repetition is bit-equal"""
    x = points("random37", n, eps, real)
    assert len(set(x[2].tolist())) == len(x[2])
    rng = np.random.default_rng(47 + n[0] + n[1] + n[2])
    ins = inputs(rng, 3, n, len(x[0]), real)
    c, f = ins[1], ins[2]
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    for sign in (-1, 1):
        m0 = run(be, plan, 1, c, sign, 0)
        assert run(be, plan, 1, c, sign, 0).tobytes() == m0.tobytes(), "a repetition differs"
        assert run(be, plan, 1, c, sign, 1).tobytes() == shift3(m0).tobytes(), "order 1 is not ifftshift of order 0"
        p0 = run(be, plan, 2, f, sign, 0)
        assert run(be, plan, 2, f, sign, 0).tobytes() == p0.tobytes(), "a repetition differs"
        assert run(be, plan, 2, shift3(f), sign, 1).tobytes() == p0.tobytes()
    perm = rng.permutation(len(x[0]))
    other = make(be, n, eps, real, table)
    set_points(be, other, tuple(v[perm] for v in x))
    m0 = run(be, plan, 1, c, -1, 0)
    assert run(be, other, 1, np.ascontiguousarray(c[:, perm]), -1, 0).tobytes() == m0.tobytes(), "permuted points give other bits"
    p0 = run(be, plan, 2, f, 1, 0)
    assert run(be, other, 2, f, 1, 0).tobytes() == np.ascontiguousarray(p0[:, perm]).tobytes()


def scaling(be, real, n, eps, x, table):
    """scaling the strengths or the modes by 2^20 and by 2^-20 scales the result exactly"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(71 + n[0])
    ins = inputs(rng, 2, n, len(x[0]), real)
    for typ in (1, 2):
        base = run(be, plan, typ, ins[typ], -1, 0)
        for s in (2.0 ** 20, 2.0 ** -20):
            scaled = (ins[typ] * ins[typ].real.dtype.type(s)).astype(ins[typ].dtype)
            assert run(be, plan, typ, scaled, -1, 0).tobytes() == (base * base.real.dtype.type(s)).astype(base.dtype).tobytes(), (real, table, typ, s)


def walk(be, real, n, eps, x, table, batch, **env):
    """both types of a handle under the development switches `env` and of one without: the pairs of results, checked against the truth"""
    rng = np.random.default_rng(53 + batch)
    ins = inputs(rng, batch, n, len(x[0]), real)
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
    note(be, real, table, f"n {n} m {len(x[0])} w {w} batch {batch} under {env}", figures)
    return res


def launch_walk(be, real, n, eps, x, table, batch, items):
    """FOURIER_LAUNCH_ITEMS splits the four new kernels' launches; the transforms' calls are the same, so every bit is"""
    res = walk(be, real, n, eps, x, table, batch, **{LAUNCH: items})
    for typ in (1, 2):
        assert res[typ][0].tobytes() == res[typ][1].tobytes(), (real, n, table, batch, items, typ, "differs from the unbounded handle")


def scratch_walk(be, real, n, eps, x, table, items):
    """batch 5 under a scratch bound of `items` fine-grid items: bit for bit the unbounded handle's result at f64, and at f32 wherever
    the number of rows ahead of every item in its launch is even in each of the three transforms under both handles.  Under the
    unbounded handle item i has i L1 L2 rows of L3 ahead of it, i L1 L3 rows of L2 in the axis-2 route and i L2 L3 rows of L1 in the
    axis-1 route: all three are even for every i where at least two of L1, L2, L3 are even.  Elsewhere the accuracy bound holds only
    (the f32 inner row kernels' last bits depend on a row's parity within its launch)"""
    L = grid(n, eps, real)
    res = walk(be, real, n, eps, x, table, 5, **{SCRATCH: items * L[0] * L[1] * L[2] * 2 * esize(real)})
    if real == "f64" or sum(l % 2 == 0 for l in L) >= 2:
        for typ in (1, 2):
            assert res[typ][0].tobytes() == res[typ][1].tobytes(), (real, n, table, items, typ, "differs from the unbounded handle")


def nan_item(be, real, n, eps, x, table):
    """a NaN strength (or mode) in one item leaves every other item bit-equal; run() checks the guard bands"""
    plan = make(be, n, eps, real, table)
    set_points(be, plan, x)
    rng = np.random.default_rng(59)
    ins = inputs(rng, RB + 1, n, len(x[0]), real)
    for typ in (1, 2):
        v = ins[typ]
        clean = run(be, plan, typ, v, -1, 0)
        bad = v.copy()
        bad.reshape(RB + 1, -1)[2, v[0].size // 2] = np.nan
        got = run(be, plan, typ, bad, -1, 0)
        assert np.isnan(got[2]).any()
        keep = [0, 1, 3, 4]
        assert got[keep].tobytes() == clean[keep].tobytes(), (real, table, typ, "a NaN in item 2 changed another item")


def history(be, real, table0):
    """one handle through a sequence of calls gives, at each call, bit for bit what a fresh handle gives for that call alone:
    set_points with 3000 points, then 37, then the ties set; both types, both signs, both orders; "table" there and back; batches 3,
    1, 7, 0, 9, 2; reserve below and above"""
    n, eps = (8, 9, 10), TIGHT[real]
    plan = make(be, n, eps, real, table0)
    rng = np.random.default_rng(83)
    table = table0
    steps = (("random3000", 3, 1, -1, 0, None, None), ("random3000", 1, 2, 1, 1, None, 2), (None, 7, 1, 1, 1, 1 - table0, None),
             ("random37", 0, 2, -1, 0, None, None), (None, 9, 2, -1, 1, None, 12), ("ties", 2, 1, -1, 0, table0, None),
             (None, 3, 2, 1, 0, None, 1), (None, 7, 1, 1, 1, None, None))
    x = None
    for name, batch, typ, sign, order, new_table, reserve in steps:
        if name is not None:
            x = points(name, n, eps, real)
            set_points(be, plan, x)
        if new_table is not None:
            table = new_table
            plan.set_option("table", table)
        if reserve is not None:
            plan.reserve(reserve)
        v = inputs(rng, batch, n, len(x[0]), real)[typ]
        if batch == 0:
            (plan.to_modes_ptr if typ == 1 else plan.to_points_ptr)(be.buf(np.zeros(4, v.dtype)).ptr, be.buf(np.zeros(4, v.dtype)).ptr, 0, sign, order)
            continue
        got = run(be, plan, typ, v, sign, order)
        fresh = make(be, n, eps, real, table)
        set_points(be, fresh, x)
        assert got.tobytes() == run(be, fresh, typ, v, sign, order).tobytes(), (real, name, batch, typ, sign, order, table, "differs from a fresh handle")
        want = want_of(typ, x, v, n, sign, order)
        note(be, real, table, f"history m {len(x[0])} w {truth.width(eps, real)} batch {batch}", [(typ, rel_l2(got, want), terms(real, n, eps, x, typ, v, sign, order, want))])


def agrees_with_2d(be, real, table):
    """at n = (20, 21, 1) the third axis holds the one mode k3 = 0, whose phase is 1 whatever x3 is: the modes equal Nufft2d's at
    (20, 21) on the same (x1, x2), within the sum of the two handles' bounds against the direct sum"""
    import nufft2d_cases as cases2

    n3, n2, eps = (20, 21, 1), (20, 21), TIGHT[real]
    x = points("random37", n3, eps, real)
    rng = np.random.default_rng(89)
    c = crand(rng, (RB + 1, len(x[0])), real)
    p3 = make(be, n3, eps, real, table)
    set_points(be, p3, x)
    p2 = cases2.make(be, n2, eps, real, table)
    cases2.set_points(be, p2, x[:2])
    for sign in (-1, 1):
        got3 = run(be, p3, 1, c, sign, 0)[..., 0]
        got2 = cases2.run(be, p2, 1, c, sign, 0)
        want = want_of(1, x, c, n3, sign, 0)
        b3 = bound(real, n3, eps, x, 1, c, sign, 0, want)
        b2 = cases2.bound(real, n2, eps, x[:2], 1, c, sign, 0, want[..., 0])
        err = rel_l2(got3, got2)
        print(f"nufft3d {be.where} {real} {ROUTES[table]} against nufft2d sign {sign}: differ by {err:.3g}, bounds {b3:.3g} + {b2:.3g}")
        assert err <= b3 + b2, (real, table, sign, err, b3, b2)


def refusals(be, real):
    """refused with INVALID and no write: a call before set_points, a NaN or infinite coordinate in any of the three arrays (the
    points stay), a null array, misaligned, in-place and overlapping buffers, a bad sign, order and option"""
    n, eps = (4, 4, 4), 1e-3
    fa = be.fa
    plan = make(be, n, eps, real)
    x = points("random37", n, eps, real)
    rng = np.random.default_rng(67)
    c = crand(rng, (2, len(x[0])), real)
    cin = be.buf(c, 0, 64)
    out = be.buf(np.full(2 * max(n[0] * n[1] * n[2], len(x[0])), SENTINEL, c.dtype))
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
    for axis in (0, 1, 2):
        bad = [v.copy() for v in x]
        bad[axis][5] = np.nan
        with pytest.raises(ValueError):
            plan.set_points(*bad)                            # the Python layer refuses it ...
        for v in (np.nan, np.inf, -np.inf):
            bad[axis][5] = v
            with pytest.raises(fa.FourierError):
                plan.set_points_ptr(*(b.ctypes.data for b in bad), len(bad[0]))  # ... and so does the library
        ptrs = [v.ctypes.data for v in x]
        ptrs[axis] = None
        with pytest.raises(fa.FourierError):
            plan.set_points_ptr(*ptrs, len(x[0]))            # a null array
        ptrs[axis] = x[axis].ctypes.data + 4
        with pytest.raises(fa.FourierError):
            plan.set_points_ptr(*ptrs, len(x[0]) - 1)        # a misaligned one
        short = list(x)
        short[axis] = x[axis][:-1]
        with pytest.raises(ValueError):
            plan.set_points(*short)
    assert plan.points() == len(x[0]) and run(be, plan, 1, c, -1, 0).tobytes() == good.tobytes(), "a refused set_points changed the points"
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
