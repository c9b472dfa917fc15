"""Every kernel, route edge and launch split behind fourier_hip_transform_axis_* (axis_plan.h, kernels_axis.h): the case tables and the
checking functions, stated once and run twice -- on the MI355X (tests/test_gpu_axis_sweep.py) and, for the subset the CPU emulation build
holds, on the emulator (tests/test_axis_sweep_emu.py).  The two callers hand in an adapter (`api`, HostApi below for the emulator) that
creates plans, makes the input of a case, runs an axis call into an output between guard elements and returns numpy arrays; shapes, routes,
truths and bounds are here.

Every small case asserts, for each transform code it runs:
  1. describe_axis(inner) names the expected route (a silent change of route fails);
  2. the out-of-place result lies between sentinel bands that are intact afterwards (the adapter's `axis`);
  3. the input is bit-unchanged (the adapter's `axis`);
  4. the in-place result is bit-equal to the out-of-place one;
  5. rel-L2 AND max_rel (helpers.py) against the truth.

Truth.  The explicit DFT matrix in np.longdouble -- cos and sin of 2 pi (jk mod N) / N formed in long double -- applied with einsum, the
scale of the scaled codes applied in long double; it depends on no FFT library.  It is rounded to complex128 where helpers.rel_l2 takes
the difference: at most 1.1e-16 of an element, against bounds of 3e-15 and more.  The column-tile cases and the N-D cases also compare
the whole array (the column tile: outer block by outer block) with numpy's FFT of the input widened to complex128.

Bounds (from the tests these transform cores already have, tests/test_gpu_tables.py, not from this sweep): lane kernels as one-launch
register kernels, rel-L2 4e-7 (f32) / 3e-15 (f64); the column tile as a tile pass, 4e-7 / 4e-15; max_rel at most twice the rel-L2 bound.
The transpose route is data movement around the plan's own batched transform: bit-equal to permute, transform_batch in place, permute
back; and the plan's own tolerance (tests/test_gpu_axis.py's tol()) against numpy, max_rel at twice that, so that a wrong composition
cannot pass by agreeing with itself."""
import concurrent.futures
import functools
import os
import re

import numpy as np

from chunk_walks import HostApi as _ChunkHostApi
from chunk_walks import same_bits
from helpers import max_rel, rel_l2

CODES = (0, 1, 2, 3, 4)  # Fft, Ifft, UnscaledIfft, SqrtScaledFft, SqrtScaledIfft (include/fourier.h)
ALL_CODES_POINTS = 1 << 21  # cases of more points run codes 0 and 1 (tests/test_gpu_axis.py's rule)
LANE_L2 = {"f32": 4e-7, "f64": 3e-15}
TILE_L2 = {"f32": 4e-7, "f64": 4e-15}
DTYPE = {"f32": np.complex64, "f64": np.complex128}
ELEM = {"f32": 8, "f64": 16}

# ---- lane route: axis_lane_kernel<T, N>, N = 1 ... 32
LANE_N = tuple(range(1, 33))
LANE_PARTS = 4  # the lengths of a test: N = part + 1, part + 5, ...
LANE_SHAPES = ((2, 3),    # (inner, outer): the smallest inner that is not the rows route
               (63, 2),   # ragged against the 64-lane wave
               (65, 5),   # ragged against the 64-lane wave; 325 lanes, not a multiple of the 256 of a workgroup
               (300, 1))

# ---- column-tile route: fft_pass_kernel<T, N, CG, MODE_LAST> launched with s = inner
COLUMN_N = (64, 128, 512, 256, 1024, 2048)
COLUMN_N_EMU = (64, 256, 1024)  # the tile-pass lengths the emulation build holds
COLUMN_OUTER = (1, 3, 11)       # at the narrowest tile: 1, 3 or 11 workgroups, ragged against the 8 XCDs of the kernel's block remap
COLUMN_WIDE = 4096
# The launch split of run_column (per = 0x7fffffff / tiles whole outer blocks a launch) takes 2^31 workgroups of at least one 16 KiB tile
# each, 32 TiB: it cannot be reached on this hardware and no case tries.

# ---- transpose route: (N, inner, outer).  Both transposes of a call run: N x inner on the way in, inner x N on the way out, so rows
# and columns of the kernel's ragged 32 x 32 edge tiles each take N mod 32 and inner mod 32.
TRANSPOSE_CASES = tuple((n, inner, 1 + 2 * ((i + k) % 2)) for i, n in enumerate((33, 63, 65, 97)) for k, inner in enumerate((2, 3, 31, 33, 65))) + (
    (64, 96, 3),     # power-of-two N, non-power-of-two inner
    (64, 2, 1),      # power-of-two inner below the narrowest tile
    (243, 40, 3),
    (1000, 100, 1),
    (4096, 7, 3))
TRANSPOSE_PARTS = 5

# ---- N-D: several routes in one fftn call: (shape, dims, [(N, inner, route prefix)] of the axis steps)
FFTN_CASES = (((2, 24, 128, 96), (1, 2, 3), ((24, 128 * 96, "axis lane: 24"), (128, 96, "axis transpose: "), (96, 1, ""))),
              ((2, 128, 64, 64), (1, 2, 3), ((128, 64 * 64, "axis column tile: L=128"), (64, 64, "axis column tile: L=64"), (64, 1, ""))))


class Worst:
    """the largest figures of one route and precision, printed by the caller"""

    def __init__(self, what):
        self.what, self.l2, self.mx, self.at_l2, self.at_mx, self.calls = what, 0.0, 0.0, None, None, 0

    def check(self, got, truth, bound, where):
        self.note(rel_l2(got, truth), max_rel(got, truth), bound, where)

    def note(self, l2, mx, bound, where):
        self.calls += 1
        if l2 >= self.l2:
            self.l2, self.at_l2 = l2, where
        if mx >= self.mx:
            self.mx, self.at_mx = mx, where
        assert l2 <= bound and mx <= 2 * bound, (self.what, where, "rel_l2", l2, "bound", bound, "max_rel", mx, "bound", 2 * bound)

    def report(self, bound):
        print(f"\naxis_sweep {self.what}: {self.calls} comparisons, worst rel_l2 {self.l2:.3g} at {self.at_l2}, worst max_rel {self.mx:.3g} "
              f"at {self.at_mx} (bounds {bound:.3g} / {2 * bound:.3g})")


# ---- the long-double truth
@functools.lru_cache(maxsize=4)
def dft_matrix(n):
    """W[k][j] = exp(-2 pi i (jk mod n) / n) in long double"""
    ld = np.longdouble
    k = np.arange(n, dtype=np.int64)
    ang = (2 * (ld(4) * np.arctan(ld(1)))) * ((k[:, None] * k[None, :]) % n).astype(ld) / ld(n)
    w = np.empty((n, n), np.clongdouble)
    w.real, w.imag = np.cos(ang), -np.sin(ang)
    w.setflags(write=False)
    return w


def code_scale_ld(code, n):
    ld = np.longdouble
    return {0: ld(1), 1: ld(1) / ld(n), 2: ld(1), 3: ld(1) / np.sqrt(ld(n)), 4: ld(1) / np.sqrt(ld(n))}[code]


def truths_ld(x, codes=CODES):
    """x: (..., N, cols) -> {code: the transform of `code` along axis -2 in long double, as complex long double}: one product with the
    matrix for the forward codes, one for the inverse ones (inverse = conj . forward . conj)"""
    n = x.shape[-2]
    w, xl = dft_matrix(n), x.astype(np.clongdouble)
    fwd = np.einsum("kj,...jc->...kc", w, xl) if set(codes) & {0, 3} else None
    inv = np.conj(np.einsum("kj,...jc->...kc", w, np.conj(xl))) if set(codes) & {1, 2, 4} else None
    return {code: (fwd if code in (0, 3) else inv) * code_scale_ld(code, n) for code in codes}


def truth_ld(x, code):
    return truths_ld(x, (code,))[code]


def truth_np(x, code):
    """numpy's FFT of x widened to complex128, along axis 1 (tests/test_gpu_axis.py's want_axis)"""
    x = x.astype(np.complex128)
    n = x.shape[1]
    y = np.fft.fft(x, axis=1) if code in (0, 3) else np.fft.ifft(x, axis=1)
    if code != 0 and code != 1:
        y *= {2: float(n), 3: 1.0 / np.sqrt(n), 4: np.sqrt(n)}[code]
    return y


def truth_fftn(x, code, dims):
    x = x.astype(np.complex128)
    if code == 0:
        return np.fft.fftn(x, axes=dims)
    if code == 3:
        return np.fft.fftn(x, axes=dims, norm="ortho")
    return np.fft.ifftn(x, axes=dims, norm={1: "backward", 2: "forward", 4: "ortho"}[code])


def plan_tol(describe, real):
    """tests/test_gpu_axis.py's tol(): one transform of the plan"""
    blu = "bluestein" in describe
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-12)


def codes_for(n, inner, outer):
    return CODES if n * inner * outer <= ALL_CODES_POINTS else (0, 1)


class HostApi:
    """the adapter of the CPU emulation build: `fa` is fourier_amd bound to it, the buffers are host memory"""
    GUARD, SENTINEL = _ChunkHostApi.GUARD, _ChunkHostApi.SENTINEL

    def __init__(self, fa):
        self.fa = fa

    def plan(self, real, n):
        return (self.fa.create_fft_f32 if real == "f32" else self.fa.create_fft_f64)(n)

    def signal(self, real, shape, seed):
        """the input of a case; .host is its numpy form (never written: every out-of-place call is checked against a kept copy)"""
        rng = np.random.default_rng(seed)
        rdt = np.float32 if real == "f32" else np.float64
        x = np.empty(shape, DTYPE[real])
        x.real, x.imag = rng.standard_normal(shape, rdt), rng.standard_normal(shape, rdt)
        return _HostSignal(x)

    def axis(self, plan, sig, code):
        """the out-of-place axis call on [outer][N][inner], into NaNs between sentinel bands: bands and input bit-unchanged afterwards.
        Returns the result as numpy"""
        x = sig.host
        outer, _, inner = x.shape
        buf = np.full(x.size + 2 * self.GUARD, self.SENTINEL, x.dtype)
        out = buf[self.GUARD:self.GUARD + x.size]
        out[:] = np.nan
        plan.transform_axis_ptr(x.ctypes.data, out.ctypes.data, outer, inner, code)
        assert np.all(buf[:self.GUARD] == self.SENTINEL) and np.all(buf[-self.GUARD:] == self.SENTINEL), "a guard element was written"
        assert same_bits(x, sig.kept), "the input of an out-of-place call was written"
        self.last = out.reshape(x.shape)
        return self.last

    def in_place_same_bits(self, plan, sig, code):
        """the in-place call on a copy of the input: bit-equal to the result axis() returned last"""
        y = sig.host.copy()
        plan.transform_axis_ptr(y.ctypes.data, y.ctypes.data, y.shape[0], y.shape[2], code)
        return same_bits(y, self.last)

    def permuted_batch_same_bits(self, plan, sig, code):
        """permute(0, 2, 1).contiguous(), the plan's own batched in-place transform of those outer * inner rows, permute back:
        bit-equal to the result axis() returned last"""
        x = sig.host
        outer, n, inner = x.shape
        rows = np.ascontiguousarray(x.transpose(0, 2, 1))
        plan.transform_batch_ptr(rows.ctypes.data, rows.ctypes.data, outer * inner, code)
        return same_bits(np.ascontiguousarray(rows.transpose(0, 2, 1)), self.last)


class _HostSignal:
    def __init__(self, x):
        self.host, self.kept = x, x.copy()


# ---- lane
def lane_lengths(part):
    return [n for n in LANE_N if (n - 1) % LANE_PARTS == part]


def lane_cases(api, real, part):
    """every (inner, outer) of LANE_SHAPES at the lengths of this part, all five codes.  N = 1: the out-of-place call is a copy (every
    scale of N = 1 is 1) and the in-place call returns before any launch; both come out as the truth says."""
    worst = Worst(f"lane {real} part {part}")
    for n in lane_lengths(part):
        plan = api.plan(real, n)
        for inner, outer in LANE_SHAPES:
            assert plan.describe_axis(inner) == f"axis lane: {n}", (n, inner, plan.describe_axis(inner))
            sig = api.signal(real, (outer, n, inner), 1000 * n + inner)
            truth = truths_ld(sig.host)
            for code in CODES:
                got = api.axis(plan, sig, code)
                assert api.in_place_same_bits(plan, sig, code), ("in place differs", real, n, inner, outer, code)
                worst.check(got, truth[code], LANE_L2[real], (n, inner, outer, code))
    worst.report(LANE_L2[real])
    return worst


# ---- column tile
def narrowest_tile(plan):
    """the smallest power of two `inner` that takes the column tile: the kernel's COLS"""
    for m in range(1, 13):
        if plan.describe_axis(1 << m).startswith("axis column tile"):
            return 1 << m
    raise AssertionError("no column tile up to inner = 4096: " + plan.describe_axis(COLUMN_WIDE))


def column_route_edges(plan, n):
    """the route around the narrowest tile `w`: transpose below it and at the non-powers of two 3 * 2^k around it, the tile from it up"""
    w = narrowest_tile(plan)
    tile, tr = f"axis column tile: L={n}", "axis transpose: " + plan.describe()
    assert 2 <= w <= 32, (n, w)
    m = 2
    while m < w:
        assert plan.describe_axis(m) == tr, (n, m, plan.describe_axis(m))
        m *= 2
    while m <= COLUMN_WIDE:
        assert plan.describe_axis(m) == tile, (n, m, plan.describe_axis(m))
        m *= 2
    for m in sorted({3 * w // 4, 3 * w // 2, 3 * w, 3 * COLUMN_WIDE // 4} - {0, 1}):
        assert m & (m - 1) and plan.describe_axis(m) == tr, (n, m, plan.describe_axis(m))
    return w


def column_samples(inner, outer, w):
    """8 columns (o, c) of a case: the first and last column of the first tile of the first block and of the last tile of the last
    block, and four in between"""
    picks = [(0, 0), (0, w - 1), (outer - 1, inner - w), (outer - 1, inner - 1)]
    tiles = inner // w
    for i, (t, c) in enumerate(((tiles // 2, 0), (tiles // 2, w - 1), (tiles // 3, w // 2), (2 * tiles // 3, w // 2 - 1))):
        picks.append(((i * outer) // 4, t * w + c))
    return picks


def block_figures(got, x, code):
    """(rel_l2, max_rel) of every outer block of `got` against numpy's f64 FFT of that block of `x`: each block is held to the bounds
    on its own, which asks no less than the whole array would (the whole array's rel-L2 is at most the largest of its blocks', and a
    block's largest value is at most the array's); the blocks go through numpy on a few threads"""
    def one(o):
        truth = truth_np(x[o:o + 1], code)
        return rel_l2(got[o:o + 1], truth), max_rel(got[o:o + 1], truth)
    if x.shape[0] == 1:
        return [one(0)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, range(x.shape[0])))


def column_cases(api, real, n, which):
    """inner = the narrowest tile (which = 0), twice that (1), 4096 (2); outer 1, 3 and 11; the whole array, block by block, against
    numpy in f64 and 8 sampled columns against the long-double matrix"""
    plan = api.plan(real, n)
    w = column_route_edges(plan, n)
    inner = (w, 2 * w, COLUMN_WIDE)[which]
    worst = Worst(f"column tile {real} N={n} inner={inner}")
    for outer in COLUMN_OUTER:
        assert plan.describe_axis(inner) == f"axis column tile: L={n}"
        sig = api.signal(real, (outer, n, inner), 7 * n + inner + outer)
        picks = column_samples(inner, outer, w)
        sample = np.stack([sig.host[o, :, c] for o, c in picks], axis=1)  # (N, 8)
        codes = codes_for(n, inner, outer)
        truth = truths_ld(sample, codes)
        for code in codes:
            got = api.axis(plan, sig, code)
            assert api.in_place_same_bits(plan, sig, code), ("in place differs", real, n, inner, outer, code)
            for o, (l2, mx) in enumerate(block_figures(got, sig.host, code)):
                worst.note(l2, mx, TILE_L2[real], (n, inner, outer, code, "numpy", "block", o))
            worst.check(np.stack([got[o, :, c] for o, c in picks], axis=1), truth[code], TILE_L2[real], (n, inner, outer, code, "long double"))
    worst.report(TILE_L2[real])
    return worst


# ---- transpose
def transpose_residues():
    """(what, residue mod 32, blocks) over both transposes of every case"""
    seen = set()
    for n, inner, outer in TRANSPOSE_CASES:
        for rows, cols in ((n, inner), (inner, n)):
            seen.add(("rows", rows % 32, outer))
            seen.add(("cols", cols % 32, outer))
    return seen


def transpose_cases(api, real, part):
    worst = Worst(f"transpose {real} part {part}")
    for n, inner, outer in TRANSPOSE_CASES[part::TRANSPOSE_PARTS]:
        plan = api.plan(real, n)
        d = plan.describe()
        assert plan.describe_axis(inner) == "axis transpose: " + d, (n, inner, plan.describe_axis(inner))
        t = plan_tol(d, real)
        sig = api.signal(real, (outer, n, inner), 13 * n + inner)
        for code in CODES:
            got = api.axis(plan, sig, code)
            assert api.in_place_same_bits(plan, sig, code), ("in place differs", real, n, inner, outer, code)
            assert api.permuted_batch_same_bits(plan, sig, code), ("not the permuted batched transform", real, n, inner, outer, code, d)
            worst.check(got, truth_np(sig.host, code), t, (n, inner, outer, code, d))
    print(f"\naxis_sweep transpose {real} part {part}: {worst.calls} calls bit-equal to permute, batched transform, permute; worst rel_l2 "
          f"{worst.l2:.3g} at {worst.at_l2}, worst max_rel {worst.mx:.3g} at {worst.at_mx} (each against its plan's own tolerance)")
    return worst


# ---- the launch splits of the large cases, restated from axis_plan.h on ITS constants
def plan_constants():
    """AXIS_SCRATCH_BYTES, AXIS_LAUNCH_BYTES and run_lane's LANES, read from fourier_amd/csrc/axis_plan.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fourier_amd", "csrc", "axis_plan.h")
    with open(path) as f:
        text = f.read()
    scratch = re.search(r"constexpr size_t AXIS_SCRATCH_BYTES = \(size_t\)1 << (\d+);", text)
    launch = re.search(r"constexpr size_t AXIS_LAUNCH_BYTES = \(\(size_t\)1 << (\d+)\) - 1;", text)
    lanes = re.search(r"const size_t LANES = \(size_t\)1 << (\d+);", text)
    assert scratch and launch and lanes, "axis_plan.h no longer states its bounds in the form this test reads"
    return {"scratch": 1 << int(scratch.group(1)), "launch": (1 << int(launch.group(1))) - 1, "lanes": 1 << int(lanes.group(1))}


def transpose_walk(n, inner, elem):
    """AxisRoute::prepare / run_transpose for one outer block: None where whole blocks fit the scratch, else per column range
    (columns, [rows of each band])"""
    k = plan_constants()
    cap = min(k["scratch"], k["launch"])
    if n * inner * elem <= cap:
        return None
    cols = max(1, cap // (n * elem))
    walk = []
    for c0 in range(0, inner, cols):
        cw = min(cols, inner - c0)
        band = min(n, (k["launch"] // elem - cw) // inner + 1)
        walk.append((cw, [min(band, n - r0) for r0 in range(0, n, band)]))
    return walk


def lane_walk(inner, outer):
    """AxisRoute::run_lane: (outer blocks, columns) of every launch"""
    lanes = plan_constants()["lanes"]
    w = min(inner, lanes)
    per = max(1, lanes // w)
    return [(min(per, outer - o0), min(w, inner - c0)) for o0 in range(0, outer, per) for c0 in range(0, inner, w)]
