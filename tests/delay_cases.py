"""The cases of the delay handle (fourier_hip_delay_*, fourier_amd.Delay) that tests/test_delay_emu.py (CPU, the emulator build) and its
`-m gpu` twin tests/test_gpu_delay.py both run, through Delay.apply_ptr on raw buffers, against tests/delay_truth.py (f64 numpy on the
inputs, delays and weights as rounded to the handle's type).  A test module passes a backend: where the buffers live.

Measure: err = ||got - want||_2 / sum_c |w_c| ||x_c||_2 per output row, the worst row of a call; rigorous for any n <= L, since every
|m| <= 1.  Bound: 3 x base -- one base for the forward transform, one for the inverse, one for the untangle and the phase, the rule by
which tests/test_gpu_conv.py takes 3 x and the cross-correlation 4 x; base is the single-transform figure of tests/test_gpu_real.py:
f32 2e-6, f64 1e-13, and 4e-6 / 1e-11 where describe() names a Bluestein plan.  An f32 numpy model of the chain gives 0.6 - 1.4e-7 at
every shape here.  Every figure is printed before it is asserted; the worst err / bound per (precision, route) is printed at module end.

Batches are 6 rows: C = 1 gives six output rows, C = 3 two groups.  The delays of every batch are delay_truth.DELAYS; weights are
absent (NULL) in some cases and uniform in [0.5, 2] in others."""
import numpy as np

import delay_truth as truth

INVALID = 1  # FOURIER_HIP_INVALID_ARGUMENT
SENTINEL = 77.0
WORST = {}   # (real, route) -> the largest err / bound seen
DEFAULT_FUSION = 1  # the handle's default of "fusion" (delay_plan.h; DESIGN.md section 4, "Fractional delay")

ONE_LAUNCH = {"f32": ((2048, 2048), (2048, 1501), (2048, 1024), (4096, 2049), (32768, 20000)),
              "f64": ((2048, 2048), (2048, 1501), (2048, 1024), (4096, 2049), (16384, 10000))}
COMPOSED = (7, 16, 255, 1000, 1031, 2048)


def ndt(real, cplx=False):
    return {("f32", False): np.float32, ("f64", False): np.float64, ("f32", True): np.complex64, ("f64", True): np.complex128}[(real, cplx)]


def has_kernel(real, L):
    return L in (2048, 4096, 8192, 16384) or (L == 32768 and real == "f32")


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


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


def make(be, n, L, real, cplx=False, channels=1, fusion=0):
    plan = be.fa.Delay(n, L, real, not cplx, channels, *((0,) if isinstance(be, DeviceBackend) else ()))
    assert (plan.size(), plan.length(), plan.channels()) == (n, L, channels)
    fused = not cplx and channels == 1 and has_kernel(real, L)
    default = "one-launch" if fused and DEFAULT_FUSION else "composed"
    assert plan.describe().startswith(f"delay {default}: "), plan.describe()
    plan.set_option("fusion", fusion)
    route = "one-launch" if fusion and fused else "composed"
    assert plan.describe().startswith(f"delay {route}: "), plan.describe()
    return plan, route


def run(be, plan, x, d, w=None, first=1, in_first=0, in_place=False):
    """apply_ptr into a buffer whose output starts on element `first` (1: an odd element) with sentinels on both sides, from an input
    that starts on element `in_first`; checks the sentinels and that the input is unmodified (in_place: the output IS the input)"""
    batch, n = x.shape
    rows = batch // plan.channels()
    xin = be.buf(x, in_first, 2)
    dl = be.buf(d)
    wt = None if w is None else be.buf(w)
    out = xin if in_place else be.buf(np.zeros(rows * n, x.dtype), first, 2)
    off = in_first if in_place else first
    before = xin.whole()
    plan.apply_ptr(xin.ptr, dl.ptr, None if wt is None else wt.ptr, out.ptr, batch)
    be.sync()
    after = out.whole()
    assert np.all(after[:off] == SENTINEL) and np.all(after[-2:] == SENTINEL), "an element beside the output was written"
    if not in_place:
        assert xin.whole().tobytes() == before.tobytes(), "apply modified its input"
    assert dl.whole().tobytes() == np.ascontiguousarray(d).tobytes()
    return after[off:off + rows * n].reshape(rows, n).copy()


def note(real, route, what, err, bound):
    print(f"delay {real} {route} {what}: err {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
    key = (real, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, (real, route, what, err, bound)


def report(where):
    for key, v in sorted(WORST.items()):
        print(f"delay {where} worst err / bound {key}: {v:.3g}")


def inputs(rng, real, n, cplx, weighted, delays=truth.DELAYS):
    batch = len(delays)
    x = truth.rows(rng, batch, n, ndt(real, cplx))
    d = np.array(delays, ndt(real))
    w = rng.uniform(0.5, 2.0, batch).astype(ndt(real)) if weighted else None
    return x, d, w


# ---- one launch: both routes against the truth and against each other, aligned and unaligned bases, in place
def one_launch(be, real, L, n, weighted):
    rng = np.random.default_rng(L + n)
    x, d, w = inputs(rng, real, n, False, weighted)
    want = truth.delay(x, d, L, 1, w)
    got = {}
    for fusion in (1, 0):
        plan, route = make(be, n, L, real, fusion=fusion)
        assert route == ("one-launch" if fusion else "composed")
        bound = 3 * base(plan, real)
        # output on an even element from an input on element 0 (f32: both 8-byte aligned), then both on an odd element
        for first, in_first in ((2, 0), (1, 1)):
            out = run(be, plan, x, d, w, first, in_first)
            note(real, route, f"L={L} n={n} weights={weighted} bases=({in_first}, {first})", truth.err(out, want, x, 1, w), bound)
            got[route, first] = out
            inp = run(be, plan, x, d, w, in_first=in_first, in_place=True)
            assert np.array_equal(inp, out), (real, L, n, route, "in place differs")
        assert np.array_equal(got[route, 2], got[route, 1]), (real, L, n, route, "the unaligned call differs from the aligned one")
    diff = truth.err(got["one-launch", 2], got["composed", 2].astype(np.float64), x, 1, w)
    note(real, "routes", f"L={L} n={n}", diff, 2 * 3 * base(plan, real))


# ---- composed: every kind of length, real and complex rows, one channel and three
def composed(be, real, cplx, channels, L):
    for i, n in enumerate(sorted({L, max(1, (3 * L + 2) // 5)})):
        rng = np.random.default_rng(100 * L + n + channels)
        weighted = (i + channels + cplx) % 2 == 1
        x, d, w = inputs(rng, real, n, cplx, weighted)
        plan, route = make(be, n, L, real, cplx, channels, 0)
        assert route == "composed"
        want = truth.delay(x, d, L, channels, w)
        out = run(be, plan, x, d, w)
        note(real, route, f"L={L} n={n} complex={cplx} C={channels} weights={weighted}", truth.err(out, want, x, channels, w), 3 * base(plan, real))
        if channels == 1:
            assert np.array_equal(run(be, plan, x, d, w, in_place=True), out), (real, cplx, L, n, "in place differs")


# ---- huge delays (f32): neither a loss of accuracy nor a fault
def huge_delays(be):
    delays = truth.DELAYS + (3e7, -1e30)
    for L, n, channels, fusion in ((2048, 1501, 1, 1), (2048, 1501, 1, 0), (1000, 600, 4, 0), (1031, 1031, 2, 0)):
        for cplx in (False, True) if not fusion else (False,):
            rng = np.random.default_rng(L + channels)
            x, d, w = inputs(rng, "f32", n, cplx, True, delays)
            plan, route = make(be, n, L, "f32", cplx, channels, fusion)
            out = run(be, plan, x, d, w)
            note("f32", route, f"huge delays L={L} n={n} complex={cplx} C={channels}",
                 truth.err(out, truth.delay(x, d, L, channels, w), x, channels, w), 3 * base(plan, "f32"))


# ---- a delay or weight that is not finite: its group's rows are not finite, nothing else is touched, and it is no error
def non_finite(be, real, fusion):
    for L, n, channels in ((2048, 1501, 1), (255, 150, 3)):
        rng = np.random.default_rng(9)
        x, d, w = inputs(rng, real, n, False, True)
        plan, route = make(be, n, L, real, False, channels, fusion)
        clean = run(be, plan, x, d, w)
        for what in ("delay nan", "delay inf", "weight nan"):
            d2, w2 = d.copy(), w.copy()
            if what == "delay nan": d2[4] = np.nan
            if what == "delay inf": d2[4] = -np.inf
            if what == "weight nan": w2[4] = np.nan
            out = run(be, plan, x, d2, w2)
            bad = 4 // channels
            assert not np.any(np.isfinite(out[bad])), (real, route, L, what)
            keep = [r for r in range(out.shape[0]) if r != bad]
            assert np.array_equal(out[keep], clean[keep]), (real, route, L, what)


# ---- exact properties
def repetition_and_scaling(be, real, fusion, channels):
    """repetition is bit-equal; the input times 2^k, or every weight times 2^k (k = -20, 20), scales the output bit for bit"""
    L, n = (2048, 1501) if fusion else (1000, 600)
    rng = np.random.default_rng(11)
    x, d, w = inputs(rng, real, n, False, True)
    plan, route = make(be, n, L, real, False, channels, fusion)
    assert route == ("one-launch" if fusion else "composed")
    out = run(be, plan, x, d, w)
    assert np.array_equal(run(be, plan, x, d, w), out), "repetition differs"
    note(real, route, f"L={L} n={n} C={channels}", truth.err(out, truth.delay(x, d, L, channels, w), x, channels, w), 3 * base(plan, real))
    for k in (-20, 20):
        s = np.asarray(2.0 ** k, x.dtype)
        scaled = (out * s).astype(out.dtype)
        assert np.array_equal(run(be, plan, x * s, d, w), scaled), (real, route, channels, k, "input scaling")
        assert np.array_equal(run(be, plan, x, d, w * s), scaled), (real, route, channels, k, "weight scaling")


def integer_delays_shift(be, real, fusion):
    """integer delays with L >= n + d: the shifted input, zeros shifting in; d = 0 without weights: the input"""
    L, n = (2048, 1501) if fusion else (1000, 600)
    rng = np.random.default_rng(12)
    x = truth.rows(rng, 6, n, ndt(real))
    d = np.array([0, 1, 5, 17, L - n, 100], ndt(real))
    plan, route = make(be, n, L, real, fusion=fusion)
    out = run(be, plan, x, d)
    want = np.zeros_like(x, dtype=np.float64)
    for r, s in enumerate(d.astype(int)):
        want[r, s:] = x[r, :n - s]
    note(real, route, f"integer delays L={L} n={n}", truth.err(out, want, x), 3 * base(plan, real))
    zero = run(be, plan, x, np.zeros(6, ndt(real)))
    note(real, route, f"zero delay L={L} n={n}", truth.err(zero, x.astype(np.float64), x), 3 * base(plan, real))


# ---- chunk and launch walks (development switches: the emulator build and the experiments library read them at create)
def group_bytes(real, cplx, channels, L):
    """the scratch of one group on the composed routes (delay_plan.h)"""
    rs = 4 if real == "f32" else 8
    spec = L if cplx else L // 2 + 1
    return (channels + (channels > 1)) * spec * 2 * rs + (0 if cplx else (channels + 1) * L * rs)


def walks(be, monkeypatch, real):
    """12 rows at C = 3 in chunks of two groups under FOURIER_DELAY_SCRATCH_BYTES; launches of one row / one group under
    FOURIER_LAUNCH_BYTES and FOURIER_LAUNCH_ITEMS at batches of 6 (C = 1) and 7 groups (C = 3): bit-equal to the unbounded handle at
    f64, and at f32 where every row keeps its parity within its launch (chunks of 6 rows do; the known deviation of the inner
    transforms, DESIGN.md "Cross-correlation")"""
    rng = np.random.default_rng(13)
    cases = []  # (switch, value, L, n, cplx, channels, groups, fusion, parity kept)
    for cplx in (False, True):
        cases.append(("FOURIER_DELAY_SCRATCH_BYTES", 2 * group_bytes(real, cplx, 3, 255) + 8, 255, 150, cplx, 3, 4, 0, True))
        cases.append(("FOURIER_LAUNCH_BYTES", 255 * 16 + 8, 255, 150, cplx, 1, 6, 0, False))
        cases.append(("FOURIER_LAUNCH_BYTES", 255 * 16 + 8, 255, 150, cplx, 3, 7, 0, False))
    cases.append(("FOURIER_DELAY_SCRATCH_BYTES", 2 * group_bytes(real, False, 3, 2048) + 8, 2048, 1501, False, 3, 4, 0, True))
    cases.append(("FOURIER_LAUNCH_ITEMS", 4, 2048, 1501, False, 1, 6, 1, True))
    for switch, value, L, n, cplx, channels, groups, fusion, parity in cases:
        batch = groups * channels
        delays = (truth.DELAYS * 4)[:batch]
        x, d, w = inputs(rng, real, n, cplx, True, delays)
        whole, _ = make(be, n, L, real, cplx, channels, fusion)
        monkeypatch.setenv(switch, str(value))
        try:
            bounded, route = make(be, n, L, real, cplx, channels, fusion)
        finally:
            monkeypatch.delenv(switch)
        a, b = run(be, whole, x, d, w), run(be, bounded, x, d, w)
        equal = np.array_equal(a, b)
        print(f"delay {real} {switch}={value} L={L} complex={cplx} C={channels} groups={groups}: bit-equal {equal}, max diff {np.abs(a - b).max():.3g}")
        note(real, route, f"{switch} L={L} complex={cplx} C={channels}", truth.err(b, truth.delay(x, d, L, channels, w), x, channels, w), 3 * base(bounded, real))
        if real == "f64" or parity:
            assert equal, (real, switch, L, cplx, channels)
