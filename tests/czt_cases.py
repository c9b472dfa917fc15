"""The cases that tests/test_czt_emu.py (CPU, emulator build) and tests/test_gpu_czt.py (MI355X) both run through fourier_amd.Czt,
against tests/czt_truth.py.  A backend supplies `run(plan, x, first=1)`: numpy rows in, the handle's output as numpy out, written into a
sentinel-bracketed buffer that starts on element `first` (1: an odd element), with the input checked unmodified.

Tolerance, relative L2 against the truth over the bins compared: base x R.  base is the Bluestein figure tests/test_gpu_real.py grants
(f32 4e-6, f64 1e-11); R is the largest over the smallest magnitude among the chirps A and B (czt_truth.chirp_ratio): 1 on the unit
circle, and the conditioning of a spiral is bounded by it.  The two routes against each other, over the WHOLE output: 2 x that bound.

Parameter sets per (n, m): "dft" w_turns = -1/m, a = 1; "zoom" w_turns = -0.1/m, a_turns = 0.2; "spiral out" / "spiral in"
w_abs = 2^(+-2 / max(n, m)^2), a_abs = 2^(1/n), on the zoom arc (R <= 4).

Bins compared with the truth: all m where n m <= 1.2e6 (every shape of L = 2048), else the 64 of helpers.sample_bins plus the two
bins at each end (the direct sum costs n x bins exact phases); the comparison of the routes always covers every bin."""
import numpy as np

import czt_truth as truth
from helpers import rel_l2, sample_bins

BASE = {"f32": 4e-6, "f64": 1e-11}
SENTINEL = 77.0
TOP = {"f32": 32768, "f64": 16384}  # the largest one-launch L


def rdt(real):
    return np.float32 if real == "f32" else np.float64


def cdt(real):
    return np.complex64 if real == "f32" else np.complex128


def next_pow2(v):
    return 1 << (int(v) - 1).bit_length()


def has_fused(real, n, m):
    return max(2048, next_pow2(n + m - 1)) <= TOP[real]


def default_route(real, n, m):
    """one launch where both routes run the same L (the measured default, profiles/czt/), else composed"""
    return "one-launch" if has_fused(real, n, m) and next_pow2(n + m - 1) >= 2048 else "composed"


def param_sets(n, m):
    """(name, w_abs, w_turns, a_abs, a_turns)"""
    s = 2.0 ** (2.0 / max(n, m) ** 2)
    return (("dft", 1.0, -1.0 / m, 1.0, 0.0), ("zoom", 1.0, -0.1 / m, 1.0, 0.2),
            ("spiral out", s, -0.1 / m, 2.0 ** (1.0 / n), 0.2), ("spiral in", 1.0 / s, -0.1 / m, 2.0 ** (1.0 / n), 0.2))


def bins_of(n, m):
    if n * m <= 1_200_000:
        return None  # all
    return sorted(set(int(k) for k in sample_bins(m)) | {0, 1, m - 2, m - 1})


def one_launch_shapes(L):
    """the smallest shapes at which each hazard of czt_small_kernel exists, for the work length L"""
    shapes = [(L // 2, L // 2 + 1),      # n + m - 1 == L: the circular wrap of v has no slack
              (L - 248, 249),            # the input reaches register rows 8 .. 15
              (200, L - 199),            # the output reaches rows 8 .. 15
              (L // 2 + 7, L // 2 - 25),  # odd lengths: 8-byte-aligned f32 rows, a ragged last unit on both sides
              (1, L), (L, 1)]            # degenerate ends
    if L == 2048:
        shapes += [(1, 1), (700, 300)]   # ... and neither side fills half
    return shapes


def real_shapes(L):
    return [(L - 248, 249), (L // 2 + 7, L // 2 - 25)]


def note(worst, real, what, route, shape, err, bound):
    print(f"czt {real} {shape} {what} {route}: err {err:.3g} bound {bound:.3g}")
    if worst is not None:
        key = (real, route)
        worst[key] = max(worst.get(key, 0.0), err / bound)
    assert err <= bound, (real, what, route, shape, err, bound)


def check(backend, fa, real, n, m, real_input=False, batch=5, sets=None, first=1, worst=None, routes=(1, 0)):
    """every parameter set on both values of "fusion" with the describe prefix asserted, against the truth; the routes against each
    other.  Returns {(set name, route): output}."""
    rng = np.random.default_rng(100003 * n + 17 * m + batch + (1 if real_input else 0))
    x = truth.rows(rng, batch, n, rdt(real) if real_input else cdt(real))
    bins = bins_of(n, m)
    results = {}
    for name, w_abs, w_turns, a_abs, a_turns in param_sets(n, m):
        if sets is not None and name not in sets:
            continue
        want = truth.czt(x, m, w_abs, w_turns, a_abs, a_turns, bins)
        bound = BASE[real] * truth.chirp_ratio(n, m, w_abs, a_abs)
        plan = fa.Czt(n, m, w_abs, w_turns, a_abs, a_turns, real, real_input, backend.device)
        assert plan.size() == n and plan.points() == m
        assert plan.describe().startswith(f"czt {default_route(real, n, m)}: "), plan.describe()
        got = {}
        for fusion in routes:
            plan.set_option("fusion", fusion)
            route = "one-launch" if fusion and has_fused(real, n, m) else "composed"
            assert plan.describe().startswith(f"czt {route}: "), plan.describe()
            out = backend.run(plan, x, first)
            assert out.shape == (batch, m)
            note(worst, real, name + (" real" if real_input else ""), route, (n, m), rel_l2(out if bins is None else out[:, bins], want), bound)
            got[route] = results[(name, route)] = out
        if len(got) == 2:
            note(worst, real, name + (" real" if real_input else ""), "routes", (n, m), rel_l2(got["one-launch"], got["composed"]), 2 * bound)
    return results
