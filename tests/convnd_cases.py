"""The cases of the N-D convolution handle (fourier_hip_convnd_*, fourier_amd.FftConvNd) that tests/test_convnd_emu.py (CPU, the
emulator build) and its `-m gpu` twin tests/test_gpu_convnd.py both run, through FftConvNd.apply_ptr on raw buffers, against
tests/convnd_truth.py (numpy rfftn / irfftn in f64 on the inputs as rounded to the handle's type).  A test module passes a backend:
where the buffers live, and which bounds hold there.

Inputs and taps are unit normal from fixed seeds, so no cancellation inflates the measure.

Measure and bound: relative L2 over the whole output of a call; three times the project's single-transform bound, because three
transforms in T contribute (the item's forward, the filter's forward, the inverse):
    GPU   f32 rank 2: 3 x 2e-6    f32 rank 3 and 4: 3 x 3e-6    f64: 3 x 1e-12     (tests/test_gpu_realnd.py's tol)
    emu   f32: 3 x 4e-6           f64: 3 x 1e-12                                   (tests/test_conv_emu.py's TOL)
    where describe() names a Bluestein plan: 3 x 4e-6 and 3 x 1e-11                (tests/test_gpu_conv.py's Bluestein values)
Every figure is printed before it is asserted; the worst err / bound per (precision, route) is printed at module end.

The shapes are the smallest at which the kernels can go wrong (MID_EDGES): h = 1; h = 2 with odd rows; odd h with the self-mirrored
row n/2; leading lengths of 1; lanes over three segments; ranks 3 and 4; odd W, which only the composed route serves."""
import numpy as np
import pytest

import convnd_truth as truth
from helpers import rel_l2

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
GUARD = 8
WORST = {}
DEFAULT_FUSION = 1  # the handle's default of "fusion" (convnd_plan.h; DESIGN.md section 4, "N-D convolution")
SCRATCH = "FOURIER_CONVND_SCRATCH_BYTES"
LAUNCH = "FOURIER_LAUNCH_ITEMS"

MID_EDGES = ([2, 2], [3, 4], [4, 6], [5, 8], [1, 16], [4, 1, 8], [3, 2304], [2, 5, 6], [3, 4, 10], [2, 3, 2, 8], [4, 7], [3, 5, 9])
LINEAR = (((7, 10), (3, 4)), ((6, 9), (4, 5)))  # (a, k) of the linear modes
MODES = ("full", "same", "valid")


def ndt(real):
    return np.float32 if real == "f32" else np.float64


def esize(real):
    return 4 if real == "f32" else 8


def has_fused(shape):
    return shape[-1] % 2 == 0


def routes(shape):
    """the values of "fusion" that give different routes"""
    return (1, 0) if has_fused(shape) else (0,)


class HostBackend:
    """buffers in host memory: the emulator build, which reads the development switches at create"""
    where = "emu"

    def __init__(self, fa, monkeypatch=None):
        self.fa, self.monkeypatch = fa, monkeypatch

    def buf(self, values, before=0, after=0):
        values = np.ascontiguousarray(values)

        class Buf:
            pass

        b = Buf()
        b.hold = np.full(values.size + before + after, SENTINEL, values.dtype)
        b.hold[before:before + values.size] = values.ravel()
        b.ptr = b.hold.ctypes.data + before * values.dtype.itemsize
        b.whole = lambda: b.hold.copy()
        return b

    def sync(self):
        pass

    def device(self):
        return -1


class DeviceBackend:
    """buffers in device memory (torch tensors); with a monkeypatch and fourier_amd bound to the experiments library, the development
    switches are read at create"""
    where = "gpu"

    def __init__(self, fa, torch, monkeypatch=None):
        self.fa, self.torch, self.monkeypatch = fa, torch, monkeypatch

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

    def device(self):
        return 0


def bound(be, plan, real):
    if "bluestein" in plan.describe().lower():
        return 3 * (4e-6 if real == "f32" else 1e-11)
    if real == "f64":
        return 3 * 1e-12
    if be.where == "emu":
        return 3 * 4e-6
    return 3 * (2e-6 if len(plan.shape()) == 2 else 3e-6)


def make(be, shape, real, fusion=DEFAULT_FUSION, **env):
    """a handle of the transform shape under the development switches `env` (read at create only), on the route of `fusion`"""
    for k, v in env.items():
        be.monkeypatch.setenv(k, str(v))
    try:
        plan = be.fa.FftConvNd(shape, real, be.device())
    finally:
        for k in env:
            be.monkeypatch.delenv(k)
    assert tuple(plan.shape()) == tuple(shape)
    default = "fused untangle" if has_fused(shape) and DEFAULT_FUSION else "composed"
    assert plan.describe().startswith(f"convnd {default}: "), plan.describe()
    plan.set_option("fusion", fusion)
    route = "fused untangle" if has_fused(shape) and fusion else "composed"
    assert plan.describe().startswith(f"convnd {route}: "), plan.describe()  # an odd W says composed under either value
    return plan, route


def set_filters(be, plan, h, correlate=False):
    """h: (F,) + k"""
    hb = be.buf(h)
    plan.set_filters_ptr(hb.ptr, h.shape[1:], h.shape[0], correlate)
    be.sync()
    assert plan.filters() == h.shape[0]


def run(be, plan, x, out_shape=None, first=0, in_place=False):
    """apply_ptr on x: (B,) + in_shape into a buffer between sentinel guard bands; checks the bands and that the input is unmodified"""
    batch = x.shape[0]
    out_shape = tuple(x.shape[1:] if out_shape is None else out_shape)
    count = batch * int(np.prod(out_shape))
    xin = be.buf(x, GUARD, GUARD)
    out = xin if in_place else be.buf(np.zeros(count, x.dtype), GUARD, GUARD)
    before = xin.whole()
    plan.apply_ptr(xin.ptr, out.ptr, batch, first)
    be.sync()
    after = out.whole()
    assert np.all(after[:GUARD] == SENTINEL) and np.all(after[-GUARD:] == SENTINEL), "an element beside the output was written"
    if not in_place:
        assert xin.whole().tobytes() == before.tobytes(), "apply modified its input"
    return after[GUARD:GUARD + count].reshape((batch,) + out_shape).copy()


def note(be, plan, real, route, what, err):
    bnd = bound(be, plan, real)
    print(f"convnd {be.where} {real} {route} {what}: err {err:.3g} bound {bnd:.3g} ratio {err / bnd:.3g}")
    key = (real, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bnd)
    assert err <= bnd, (real, route, what, err, bnd)


def report(where):
    for key, v in sorted(WORST.items()):
        print(f"convnd {where} worst err / bound {key}: {v:.3g}")


def rand(rng, shape, real):
    return np.ascontiguousarray(rng.standard_normal(shape).astype(ndt(real)))


# ---- the mid kernel's edges, and the banks: F = 1; F = 3 with batch 5 and filter_first 2 (the index wraps twice); both routes, which
# must also agree with each other; in place under the whole window
def mid_edges(be, real, shape, batch=5):
    rng = np.random.default_rng(sum(shape) + len(shape))
    shape = tuple(shape)
    x = rand(rng, (batch,) + shape, real)
    k = tuple(min(3, n) for n in shape)
    banks_ = [(rand(rng, (F,) + k, real), first, correlate) for F, first, correlate in ((1, 0, False), (3, 2, False), (3, 2, True))]
    got = {}
    for fusion in routes(shape):
        plan, route = make(be, shape, real, fusion)
        for i, (h, first, correlate) in enumerate(banks_):
            set_filters(be, plan, h, correlate)
            y = run(be, plan, x, first=first)
            note(be, plan, real, route, f"{list(shape)} F={h.shape[0]} first={first} correlate={correlate}",
                 rel_l2(y, truth.circular(x, h, shape, correlate, first)))
            assert run(be, plan, x, first=first, in_place=True).tobytes() == y.tobytes(), (shape, route, "in place differs")
            if i in got:
                note(be, plan, real, "fused untangle", f"{list(shape)} F={h.shape[0]} against the composed route", rel_l2(got[i], y))
            got[i] = y


def banks(be, real, fusion):
    """taps of the whole shape and of [1, ..., 1]; a delta returns the input; a delta at (1, 2) is np.roll; correlate is the conjugated
    spectrum, that is the roll the other way"""
    rng = np.random.default_rng(11)
    for shape in ((4, 6), (3, 4, 10)):
        plan, route = make(be, shape, real, fusion)
        r = len(shape)
        x = rand(rng, (3,) + shape, real)
        for k in (shape, (1,) * r):
            h = rand(rng, (2,) + k, real)
            set_filters(be, plan, h)
            note(be, plan, real, route, f"{list(shape)} taps {list(k)}", rel_l2(run(be, plan, x), truth.circular(x, h, shape)))
        set_filters(be, plan, np.ones((1,) + (1,) * r, ndt(real)))
        note(be, plan, real, route, f"{list(shape)} delta", rel_l2(run(be, plan, x), x))
        h = np.zeros((1,) + (1,) * (r - 2) + (2, 3), ndt(real))
        h[(0,) * (r - 1) + (1, 2)] = 1
        set_filters(be, plan, h)
        note(be, plan, real, route, f"{list(shape)} delta at (1, 2)", rel_l2(run(be, plan, x), np.roll(x, (1, 2), axis=(-2, -1))))
        set_filters(be, plan, h, correlate=True)
        y = run(be, plan, x)
        note(be, plan, real, route, f"{list(shape)} delta at (1, 2), correlate", rel_l2(y, np.roll(x, (-1, -2), axis=(-2, -1))))
        note(be, plan, real, route, f"{list(shape)} correlate against the conjugated spectrum", rel_l2(y, truth.circular(x, h, shape, True)))


def windows(be, real, fusion):
    """in_shape < S in every dimension and in one only; a window inside S; back to the default"""
    rng = np.random.default_rng(13)
    for shape, ins in (((5, 8), ((3, 5), (5, 7), (4, 8))), ((3, 4, 10), ((2, 3, 7), (3, 2, 10))), ((4, 7), ((3, 4), (4, 6)))):
        if fusion and not has_fused(shape):
            continue
        plan, route = make(be, shape, real, fusion)
        h = rand(rng, (2,) + tuple(min(2, n) for n in shape), real)
        set_filters(be, plan, h)
        for a in ins:
            x = rand(rng, (3,) + a, real)
            full = truth.circular(x, h, shape, False, 1)
            plan.set_window(a, None, None)
            note(be, plan, real, route, f"{list(shape)} in {list(a)}", rel_l2(run(be, plan, x, shape, first=1), full))
            fst = tuple(min(1, n - 1) for n in shape)
            size = tuple(n - f - (1 if n - f > 1 else 0) for n, f in zip(shape, fst))
            plan.set_window(a, fst, size)
            note(be, plan, real, route, f"{list(shape)} in {list(a)} window {list(fst)} + {list(size)}",
                 rel_l2(run(be, plan, x, size, first=1), truth.window(full, fst, size)))
        plan.set_window()
        x = rand(rng, (3,) + shape, real)
        note(be, plan, real, route, f"{list(shape)} default window again", rel_l2(run(be, plan, x), truth.circular(x, h, shape)))


def linear_modes(be, real, fusion):
    """the windows of scipy.signal.convolve's three modes on the handle, against the circular truth and against scipy's direct sums"""
    rng = np.random.default_rng(17)
    for a, k in LINEAR:
        shape = tuple(be.fa.next_fast_len(n + m - 1, even=(d == 1)) for d, (n, m) in enumerate(zip(a, k)))
        plan, route = make(be, shape, real, fusion)
        x = rand(rng, (4,) + a, real)
        h = rand(rng, (3,) + k, real)
        set_filters(be, plan, h)
        for mode in MODES:
            fst, size = truth.linear_window(a, k, mode)
            plan.set_window(a, fst, size)
            y = run(be, plan, x, size)
            note(be, plan, real, route, f"a={a} k={k} {mode} against the circular truth", rel_l2(y, truth.window(truth.circular(x, h, shape), fst, size)))
            note(be, plan, real, route, f"a={a} k={k} {mode} against scipy", rel_l2(y, truth.scipy_linear(x, h, mode)))


# ---- walks: a handle under a development switch against a handle without, and against the truth
def walk(be, real, shape, fusion, batch, windowed, **env):
    rng = np.random.default_rng(19 + batch)
    shape = tuple(shape)
    a = tuple(max(1, n - 1) for n in shape) if windowed else shape
    fst = tuple(min(1, n - 1) for n in shape) if windowed else (0,) * len(shape)
    size = tuple(n - f for n, f in zip(shape, fst))
    x = rand(rng, (batch,) + a, real)
    h = rand(rng, (3,) + tuple(min(2, n) for n in shape), real)
    ys = []
    for e in (env, {}):
        plan, route = make(be, shape, real, fusion, **e)
        plan.set_window(a, fst, size)
        set_filters(be, plan, h)
        ys.append(run(be, plan, x, size, first=1))
    note(be, plan, real, route, f"{list(shape)} batch {batch} under {env}", rel_l2(ys[0], truth.window(truth.circular(x, h, shape, False, 1), fst, size)))
    return ys, plan, route


def item_bytes(shape, real, fusion):
    """scratch bytes per item of a chunk (convnd_plan.h): the packed rows in a half spectrum's size; twice that on the composed route"""
    rows = int(np.prod(shape[:-1]))
    return (1 if fusion and has_fused(shape) else 2) * rows * (shape[-1] // 2 + 1) * 2 * esize(real)


def scratch_walk(be, real, shape, fusion, items, windowed):
    """batch 5 under a scratch bound of `items` items: bit for bit the unbounded handle's result at f64, and at f32 where a chunk holds
    an even number of rows (the known parity deviation of the f32 inner transforms); else within the bound"""
    ys, plan, route = walk(be, real, shape, fusion, 5, windowed, **{SCRATCH: items * item_bytes(shape, real, fusion)})
    rows = items * int(np.prod(shape[:-1]))
    if real == "f64" or rows % 2 == 0:
        assert ys[0].tobytes() == ys[1].tobytes(), (real, shape, route, items, "differs from the unbounded handle")
    else:
        note(be, plan, real, route, f"{list(shape)} chunks of {items} against the unbounded handle", rel_l2(ys[0], ys[1]))


def launch_walk(be, real, shape, fusion, batch, windowed):
    """FOURIER_LAUNCH_ITEMS = 1 splits every new sweep into launches of one item; the transforms' calls are the same, so every bit is"""
    ys, _, route = walk(be, real, shape, fusion, batch, windowed, **{LAUNCH: 1})
    assert ys[0].tobytes() == ys[1].tobytes(), (real, shape, route, batch, "differs from the unbounded handle")


# ---- the argument checks that need a handle
def argument_checks(be, real):
    shape = (4, 6)
    plan, _ = make(be, shape, real)
    x = rand(np.random.default_rng(23), (2,) + shape, real)
    xin, out = be.buf(x), be.buf(np.zeros_like(x))
    e = esize(real)
    fa = be.fa
    raises = pytest.raises
    with raises(fa.FourierError):                         # apply before set_filters
        plan.apply_ptr(xin.ptr, out.ptr, 2)
    h = be.buf(np.ones((2, 2, 3), ndt(real)))
    for bad in ((0, 3), (2, 7), (5, 3)):                  # a length of 0, and lengths above S
        with raises(fa.FourierError):
            plan.set_filters_ptr(h.ptr, bad, 1)
    with raises(fa.FourierError):
        plan.set_filters_ptr(h.ptr, (2, 3), 0)            # no filters
    with raises(fa.FourierError):
        plan.set_filters_ptr(0, (2, 3), 1)                # null
    with raises(fa.FourierError):
        plan.set_filters_ptr(h.ptr + 2, (2, 3), 1)        # taps are aligned to one value
    with raises(ValueError):
        plan.set_filters_ptr(h.ptr, (2, 3, 1), 1)         # the rank
    assert plan.filters() == 0
    plan.set_filters_ptr(h.ptr, (2, 3), 2)
    assert plan.filters() == 2
    plan.apply_ptr(xin.ptr, out.ptr, 2)
    plan.apply_ptr(xin.ptr, xin.ptr, 2)                   # in place under the whole window
    plan.apply_ptr(xin.ptr, out.ptr, 0)                   # batch 0: a no-op
    for a, b in ((0, out.ptr), (xin.ptr, 0), (xin.ptr + e, out.ptr), (xin.ptr, out.ptr + e), (xin.ptr, xin.ptr + 2 * e)):
        with raises(fa.FourierError):                     # null, aligned to one real only (2 needed), partial overlap
            plan.apply_ptr(a, b, 2)
    with raises(fa.FourierError):
        plan.apply_ptr(xin.ptr, out.ptr, 1 << 62)         # oversize
    # set_window's bounds: a length of 0, above S, a window that would wrap
    for win in (((0, 6), None, None), ((5, 6), None, None), (None, None, (4, 7)), (None, (1, 0), None), (None, (0, 3), (4, 4)), (None, None, (0, 6))):
        with raises(fa.FourierError):
            plan.set_window(*win)
    plan.apply_ptr(xin.ptr, out.ptr, 2)                   # a refused window leaves the old one
    plan.set_window((3, 5), (1, 2), (3, 4))
    small = be.buf(np.zeros((2, 3, 5), ndt(real)), 0, 64)
    with raises(fa.FourierError):
        plan.apply_ptr(small.ptr, small.ptr, 2)           # in place under a window
    with raises(fa.FourierError):
        plan.apply_ptr(small.ptr, small.ptr + 4 * e, 2)   # overlapping under a window
    plan.apply_ptr(small.ptr, out.ptr, 2)
    for key, v in (("fusion", 2), ("no_such_option", 1)):
        with raises(fa.FourierError):
            plan.set_option(key, v)
    be.sync()
