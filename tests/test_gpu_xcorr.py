"""The cross-correlation handle on the MI355X: fourier_hip_xcorr_* through fourier_amd.CrossCorrelation and xcorr / gcc_phat on torch
tensors, against tests/xcorr_truth.py (f64 numpy on the rounded inputs).  The CPU twin is tests/test_xcorr_emu.py (it also covers the
argument checks of the C ABI and the allocation-free property after reserve); the measure and the tolerances are stated there:
||got - want_window||_2 / ||want over all L lags||_2 against 4 x base (no weighting, white rows) or base x (sqrt(2 (kx^2 + ky^2)) + 1)
(PHAT, spike rows, kx, ky <= 3 asserted, the peak at the delay asserted).

The product's one-launch table holds the kernels without scratch memory (f64, no weighting); the others run here through the
experiments library under its development switch FOURIER_XCORR_SPILLING (`lib` = "experiments"), so that every instance runs on the
GPU, and the product library (`lib` = "product") is checked with the table it ships.

Sizes: L = 2048 and 4096 (the two smallest L1 x L2 shapes of the one-launch kernel), 32768 at f32 and 16384 at f64 (the largest), n in
(L, L/2), four windows, both weightings, batch 5; one batch of 1025 pairs at L = 2048, more workgroups than one per CU; L in (1, 2, 255,
1000, 1031) real and complex and 2048 complex on the composed route only.  Every figure is printed before it is asserted; the worst err
/ bound per (precision, weighting, route) is printed at module end.  Every case runs once."""
import numpy as np
import pytest

import xcorr_truth as truth

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
DELAY = 2
WORST = {}


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU: the product path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def fa(torch):
    import fourier_amd
    from fourier_amd import _lib

    _lib.lib()
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read()
    yield fourier_amd
    for key, v in sorted(WORST.items()):
        print(f"xcorr gpu worst err / bound {key}: {v:.3g}")


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test (tests/test_gpu_chunks.py): it reads the development switches from
    the environment at create.  A handle keeps the library it was created from."""
    import ctypes
    import os

    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


def tdt(torch, real, cplx=False):
    return {("f32", False): torch.float32, ("f64", False): torch.float64, ("f32", True): torch.complex64, ("f64", True): torch.complex128}[(real, cplx)]


def ndt(real, cplx=False):
    return {("f32", False): np.float32, ("f64", False): np.float64, ("f32", True): np.complex64, ("f64", True): np.complex128}[(real, cplx)]


def base(plan, real):
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def has_kernel(spilling, real, L, phat):
    shape = L in (2048, 4096, 8192, 16384) or (L == 32768 and real == "f32")
    return shape and (spilling or (real == "f64" and not phat))


def windows(L, n):
    w = [(0, L), (-3, 7), (L - 2, 6)]
    if 2 * n - 1 <= L:
        w.insert(1, (-(n - 1), 2 * n - 1))
    return w


def make(mod, monkeypatch, spilling, n, L, first, lags, real, cplx=False, phat=False, fusion=0):
    if spilling:
        monkeypatch.setenv("FOURIER_XCORR_SPILLING", "1")
    try:
        plan = mod.CrossCorrelation(n, L, first, lags, real, not cplx, 0)
    finally:
        if spilling:
            monkeypatch.delenv("FOURIER_XCORR_SPILLING")
    default = "one-launch" if not cplx and has_kernel(spilling, real, L, False) else "composed"  # (no weighting yet)
    assert plan.describe().startswith(f"xcorr {default}: "), plan.describe()
    plan.set_option("weighting", int(phat))
    plan.set_option("fusion", fusion)
    route = "one-launch" if fusion and not cplx and has_kernel(spilling, real, L, phat) else "composed"
    assert plan.describe().startswith(f"xcorr {route}: "), plan.describe()
    return plan, route


def run(torch, plan, x, y, first=1):
    """into a buffer whose output starts on element `first` (1: an odd element) with sentinels on both sides; checks them and that the
    inputs are unmodified"""
    kx, ky = x.clone(), y.clone()
    count = x.shape[0] * plan.lags()
    buf = torch.full((count + first + 2,), SENTINEL, dtype=x.dtype, device="cuda")
    out = buf[first:first + count].view(x.shape[0], plan.lags())
    assert plan.correlate(x, y, out=out) is out
    assert torch.all(buf[:first] == SENTINEL).item() and torch.all(buf[-2:] == SENTINEL).item(), "an element beside the output was written"
    assert torch.equal(x, kx) and torch.equal(y, ky), "correlate modified an input"
    return out.cpu().numpy()


def note(real, weighting, route, what, err, bound):
    print(f"xcorr {real} {weighting} {route} {what}: err {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
    key = (real, weighting, route)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, (real, weighting, route, what, err, bound)


def check(torch, mod, monkeypatch, spilling, real, L, n, batch, cplx=False, fusions=(1, 0)):
    rng = np.random.default_rng(1000 * batch + L + n)
    d = DELAY if n > 2 * DELAY else 0
    for phat in (False, True):
        if phat:
            xh, yh = truth.spike_rows(rng, batch, n, d, ndt(real, cplx))
            kx, ky = truth.kappa(xh, L), truth.kappa(yh, L)
            assert kx <= 3 and ky <= 3, (kx, ky)  # a condition on the inputs
        else:
            xh, yh = truth.rows(rng, batch, n, ndt(real, cplx)), truth.rows(rng, batch, n, ndt(real, cplx))
        x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
        want = truth.full(xh, yh, L, phat)
        name = "phat" if phat else "none"
        for first, lags in windows(L, n) if L >= 8 else [(0, L)]:
            got = {}
            for fusion in fusions:
                plan, route = make(mod, monkeypatch, spilling, n, L, first, lags, real, cplx, phat, fusion)
                bound = base(plan, real) * ((np.sqrt(2 * (kx * kx + ky * ky)) + 1) if phat else 4)
                out = run(torch, plan, x, y)
                note(real, name, route, f"L={L} n={n} window=({first}, {lags}) batch={batch}", truth.window_err(out, want, first, lags), bound)
                if phat and (d - first) % L < lags:
                    assert np.all(np.argmax(np.abs(out), axis=-1) == (d - first) % L), (real, L, n, first, lags, route)
                got[route] = out, bound
            if len(got) == 2:
                diff = np.linalg.norm(got["one-launch"][0] - got["composed"][0]) / np.linalg.norm(want)
                note(real, name, "routes", f"L={L} n={n} window=({first}, {lags})", diff, 2 * max(got["one-launch"][1], got["composed"][1]))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_both_routes_of_the_product(torch, fa, monkeypatch, real):
    """the table the product ships: "fusion" = 1 is the one-launch kernel at f64 without weighting and the composed route elsewhere"""
    for L in (2048, 4096, 32768 if real == "f32" else 16384):
        for n in (L, L // 2):
            check(torch, fa, monkeypatch, False, real, L, n, 5)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_both_routes_with_every_one_launch_instance(torch, fx, monkeypatch, real):
    for L in (2048, 4096, 32768 if real == "f32" else 16384):
        for n in (L, L // 2):
            check(torch, fx, monkeypatch, True, real, L, n, 5)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_one_per_cu(torch, fx, monkeypatch, real):
    check(torch, fx, monkeypatch, True, real, 2048, 1024, 1025)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
def test_composed_only_shapes(torch, fa, monkeypatch, real, cplx):
    for L in (1, 2, 255, 1000, 1031):
        for n in sorted({L, (L + 1) // 2}):
            check(torch, fa, monkeypatch, False, real, L, n, 5, cplx, fusions=(0,))
    if cplx:  # complex rows have no one-launch route: "fusion" = 1 stays composed
        plan, route = make(fa, monkeypatch, False, 2048, 2048, 0, 2048, real, True, False, 1)
        assert route == "composed" and "complex rows" in plan.describe()
        check(torch, fa, monkeypatch, False, real, 2048, 1024, 5, True, fusions=(1,))
    else:
        plan, route = make(fa, monkeypatch, False, 32768, 32768, 0, 32768, "f64", fusion=1)  # no f64 kernel of that length
        assert route == "composed" and "no one-launch kernel" in plan.describe()


@pytest.mark.parametrize("fusion", [1, 0])
@pytest.mark.parametrize("phat", [False, True])
def test_f32_bases_that_are_only_4_byte_aligned(torch, fx, monkeypatch, fusion, phat):
    """the element-wise loads and stores of the one-launch kernel (and the composed route on the same pointers), for x, y and out:
    bit-equal to the aligned call"""
    L, n, batch = 2048, 1024, 5
    rng = np.random.default_rng(6)
    xh, yh = truth.spike_rows(rng, batch, n, DELAY, np.float32)
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()

    def shifted(v):
        holder = torch.zeros(v.numel() + 1, dtype=torch.float32, device="cuda")
        s = holder[1:].view(v.shape)
        s.copy_(v)
        assert v.data_ptr() % 8 == 0 and s.data_ptr() % 8 == 4
        return s

    for first, lags in ((0, L), (-(n - 1), 2 * n - 2), (-4, 8)):
        plan, route = make(fx, monkeypatch, True, n, L, first, lags, "f32", False, phat, fusion)
        aligned = run(torch, plan, x, y, first=2)
        for xx, yy, o in ((shifted(x), y, 2), (x, shifted(y), 2), (x, y, 1), (shifted(x), shifted(y), 1)):
            assert np.array_equal(run(torch, plan, xx, yy, first=o), aligned), (route, first, lags)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("route", ["one-launch", "composed"])
def test_power_of_two_scaling(torch, fx, monkeypatch, real, route):
    """x * 2^20, y * 2^-30: the unweighted output is bit-equal to 2^-10 x the unscaled result, the PHAT output bit-identical"""
    n = L = 2048
    rng = np.random.default_rng(5)
    xh, yh = truth.spike_rows(rng, 5, n, DELAY, ndt(real))
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
    xs, ys = x * 2.0 ** 20, y * 2.0 ** -30
    for phat in (False, True):
        plan, got = make(fx, monkeypatch, True, n, L, 0, L, real, False, phat, int(route == "one-launch"))
        assert got == route
        plain, scaled = run(torch, plan, x, y), run(torch, plan, xs, ys)
        want = truth.full(xs.cpu().numpy(), ys.cpu().numpy(), L, phat)
        bound = base(plan, real) * (4 if not phat else np.sqrt(2 * (truth.kappa(xh, L) ** 2 + truth.kappa(yh, L) ** 2)) + 1)
        note(real, "phat" if phat else "none", route, "scaled rows", truth.window_err(scaled, want, 0, L), bound)
        assert np.array_equal(scaled, plain if phat else (plain * 2.0 ** -10).astype(plain.dtype)), (real, route, phat)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_all_zero_row_under_phat_gives_exact_zeros(torch, fx, monkeypatch, real, fusion):
    rng = np.random.default_rng(4)
    for L, n in ((2048, 1024), (100, 100)):
        xh, yh = truth.spike_rows(rng, 5, n, DELAY, ndt(real))
        xh[1] = 0
        yh[2] = 0
        xh[3] = 0
        yh[3] = 0
        plan, _ = make(fx, monkeypatch, True, n, L, 0, L, real, False, True, fusion)
        out = run(torch, plan, torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda())
        assert np.all(np.isfinite(out)) and np.all(out[1:4] == 0) and np.any(out[0] != 0) and np.any(out[4] != 0)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_walk_equals_the_one_chunk_result(torch, fx, real, monkeypatch):
    """a handle created under a bound of two row pairs of scratch walks 5 rows in 3 chunks: bit-equal to a handle of the same library
    without the bound"""
    rs, cs = (4, 8) if real == "f32" else (8, 16)
    rng = np.random.default_rng(7)
    for L, n, cplx in ((255, 128, False), (2048, 1024, False), (255, 128, True)):
        x = torch.from_numpy(truth.rows(rng, 5, n, ndt(real, cplx))).cuda()
        y = torch.from_numpy(truth.rows(rng, 5, n, ndt(real, cplx))).cuda()
        per = 2 * L * cs if cplx else 2 * (L // 2 + 1) * cs + 3 * L * rs  # the scratch of one row pair (xcorr_plan.h)
        for phat in (False, True):
            for first, lags in ((0, L), (-3, 7)):
                whole, _ = make(fx, monkeypatch, False, n, L, first, lags, real, cplx, phat)
                monkeypatch.setenv("FOURIER_XCORR_SCRATCH_BYTES", str(2 * per + 8))
                try:
                    small, _ = make(fx, monkeypatch, False, n, L, first, lags, real, cplx, phat)
                finally:
                    monkeypatch.delenv("FOURIER_XCORR_SCRATCH_BYTES")
                a, b = run(torch, whole, x, y), run(torch, small, x, y)
                assert np.array_equal(a, b), (real, L, cplx, phat, first)
                if not phat:
                    note(real, "none", "composed chunks", f"L={L} window=({first}, {lags})",
                         truth.window_err(b, truth.full(x.cpu().numpy(), y.cpu().numpy(), L), first, lags), 4 * base(small, real))


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, monkeypatch, fusion):
    """correlate captured on a side stream as the first call of a handle that reserved (it must not allocate), one linear graph,
    replayed twice on new input contents: bit-equal to the eager call.  f64: the precision whose one-launch kernel the product runs."""
    L, n, batch = 2048, 1024, 5
    rng = np.random.default_rng(20)
    xs = [torch.from_numpy(truth.rows(rng, batch, n, np.float64)).cuda() for _ in range(3)]
    ys = [torch.from_numpy(truth.rows(rng, batch, n, np.float64)).cuda() for _ in range(3)]
    side = torch.cuda.Stream()
    other, _ = make(fa, monkeypatch, False, n, L, -(n - 1), 2 * n - 1, "f64", fusion=fusion)  # loads the kernels' code object
    with torch.cuda.stream(side):
        other.correlate(xs[0], ys[0])
    side.synchronize()
    plan, route = make(fa, monkeypatch, False, n, L, -(n - 1), 2 * n - 1, "f64", fusion=fusion)
    assert route == ("one-launch" if fusion else "composed")
    plan.reserve(batch)
    torch.cuda.synchronize()
    dx, dy = xs[0].clone(), ys[0].clone()
    out = torch.empty(batch, 2 * n - 1, dtype=torch.float64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.correlate(dx, dy, out=out)  # the first call on this plan: captured
    for x, y in zip(xs[1:], ys[1:]):
        dx.copy_(x)
        dy.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        eager = plan.correlate(x, y)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), fusion
        want = truth.full(x.cpu().numpy(), y.cpu().numpy(), L)
        note("f64", "none", route, "graph replay", truth.window_err(out.cpu().numpy(), want, -(n - 1), 2 * n - 1), 4 * base(plan, "f64"))


def test_torch_layer(torch, fa):
    rng = np.random.default_rng(9)
    for real in ("f32", "f64"):
        rt, ct = tdt(torch, real), tdt(torch, real, True)
        n = 300
        xh, yh = truth.rows(rng, 6, n, ndt(real)), truth.rows(rng, 6, n, ndt(real))
        x, y = torch.from_numpy(xh).cuda().view(2, 3, n), torch.from_numpy(yh).cuda().view(2, 3, n)
        tol = 4 * (2e-6 if real == "f32" else 1e-13)
        # xcorr against numpy.correlate(y, x, "full"): lags -(n - 1) ... n - 1
        r = fa.xcorr(x, y)
        assert r.shape == (2, 3, 2 * n - 1) and r.dtype == rt
        want = np.stack([np.correlate(yh[i].astype(np.float64), xh[i].astype(np.float64), "full") for i in range(6)])
        got = r.reshape(6, -1).cpu().numpy()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= tol, real
        assert list(fa.correlation_lags(n)) == list(range(-(n - 1), n))
        # the module function against the handle, bit for bit; out=
        plan = fa.CrossCorrelation(n, 1024, -(n - 1), 2 * n - 1, real, True, 0)
        assert torch.equal(r, plan.correlate(x, y))
        out = torch.empty(2, 3, 2 * n - 1, dtype=rt, device="cuda")
        assert fa.xcorr(x, y, out=out) is out and torch.equal(out, r)
        assert plan.correlate(x[0, 0], y[0, 0]).shape == (2 * n - 1,)
        # max_lag: the centred window
        m = fa.xcorr(x, y, max_lag=10)
        assert m.shape == (2, 3, 21) and list(fa.correlation_lags(n, 10)) == list(range(-10, 11))
        assert np.linalg.norm(m.reshape(6, -1).cpu().numpy() - want[:, n - 11:n + 10]) / np.linalg.norm(want) <= tol
        # circular: the raw order, and the centred window
        c = fa.xcorr(x, y, mode="circular")
        cw = truth.full(xh, yh, n)
        assert c.shape == x.shape and np.linalg.norm(c.reshape(6, -1).cpu().numpy() - cw) / np.linalg.norm(cw) <= tol
        c5 = fa.xcorr(x, y, max_lag=5, mode="circular")
        assert c5.shape == (2, 3, 11) and np.linalg.norm(c5.reshape(6, -1).cpu().numpy() - truth.window(cw, -5, 11)) / np.linalg.norm(cw) <= tol
        # gcc_phat: the peak at the delay
        sx, sy = truth.spike_rows(rng, 4, n, 7, ndt(real))
        g = fa.gcc_phat(torch.from_numpy(sx).cuda(), torch.from_numpy(sy).cuda(), max_lag=20)
        assert g.shape == (4, 41) and torch.all(torch.argmax(g, dim=-1) == 27).item()
        assert torch.equal(g, fa.xcorr(torch.from_numpy(sx).cuda(), torch.from_numpy(sy).cuda(), max_lag=20, weighting="phat"))
        # complex rows: complex output, conj on x
        zx, zy = truth.rows(rng, 3, 100, ndt(real, True)), truth.rows(rng, 3, 100, ndt(real, True))
        z = fa.xcorr(torch.from_numpy(zx).cuda(), torch.from_numpy(zy).cuda())
        zw = np.stack([np.correlate(zy[i].astype(np.complex128), zx[i].astype(np.complex128), "full") for i in range(3)])
        assert z.dtype == ct and np.linalg.norm(z.cpu().numpy() - zw) / np.linalg.norm(zw) <= tol
        # a non-last dim: the axis moved last, correlated, moved back; and a non-contiguous layout
        t, u = x.transpose(0, 2).contiguous(), y.transpose(0, 2).contiguous()  # (n, 3, 2)
        got0 = fa.xcorr(t, u, dim=0)
        # (the rows run in another order, and the f32 transforms' last bits depend on a row's position: within tolerance, not bit for bit)
        assert got0.shape == (2 * n - 1, 3, 2)
        assert np.linalg.norm(got0.cpu().numpy().transpose(2, 1, 0).reshape(6, -1) - want) / np.linalg.norm(want) <= tol
        nc = fa.xcorr(x.transpose(0, 1), y.transpose(0, 1))
        assert nc.shape == (3, 2, 2 * n - 1)
        assert np.linalg.norm(nc.transpose(0, 1).reshape(6, -1).cpu().numpy() - want) / np.linalg.norm(want) <= tol
        # x is y: the autocorrelation
        a = fa.xcorr(x, x, max_lag=3)
        assert torch.all(torch.argmax(a, dim=-1) == 3).item()
        # the refusals
        with pytest.raises(TypeError):
            plan.correlate(x, y, out=torch.empty(2, 3, 2 * n - 1, dtype=rt))                 # not on the device
        with pytest.raises(TypeError):
            plan.correlate(x, y, out=torch.empty(2, 3, 2 * n - 1, dtype=ct, device="cuda"))  # not the inputs' dtype
        with pytest.raises(TypeError):
            plan.correlate(x, y, out=torch.empty(6, 2 * n - 1, dtype=rt, device="cuda"))     # not the inputs' shape
        with pytest.raises(ValueError):
            plan.correlate(x[..., :299].contiguous(), y[..., :299].contiguous())             # the wrong last dimension
        with pytest.raises(ValueError):
            plan.correlate(x, y[:1])                                                         # x and y of different shape
        with pytest.raises(TypeError):
            plan.correlate(x, y.to(torch.float64 if real == "f32" else torch.float32))       # ... or dtype
        big = torch.zeros(6 * (2 * n - 1) + 6 * n, dtype=rt, device="cuda")
        with pytest.raises(fa.FourierError):
            plan.correlate(big[:6 * n].view(6, n), y.view(6, n), out=big[n:n + 6 * (2 * n - 1)].view(6, 2 * n - 1))  # partial overlap
    x = torch.zeros(4, 100, dtype=torch.float32, device="cuda")
    for fn in (fa.xcorr, fa.gcc_phat):
        with pytest.raises(TypeError):
            fn(x.cpu(), x.cpu())
        with pytest.raises(TypeError):
            fn(x, x.to(torch.float64))
        with pytest.raises(TypeError):
            fn(x.to(torch.int32), x.to(torch.int32))
        with pytest.raises(TypeError):
            fn(x, x, out=torch.empty(4, 198, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            fn(x, x[:2])
        with pytest.raises(ValueError):
            fn(x[:, :0], x[:, :0])
        with pytest.raises(ValueError):
            fn(x, x, dim=2)
        with pytest.raises(ValueError):
            fn(x, x, max_lag=100)
        with pytest.raises(ValueError):
            fn(x, x, max_lag=50, mode="circular")
        with pytest.raises(ValueError):
            fn(x, x, mode="valid")
    with pytest.raises(ValueError):
        fa.xcorr(x, x, weighting="scot")
    with pytest.raises(ValueError):
        fa.CrossCorrelation(0, 8, 0, 8, "f32", True, 0)


def test_f32_last_bits_depend_on_a_rows_parity_in_the_inner_transforms(torch, fx, monkeypatch):
    """The known deviation from "bit-equal under any scratch bound" (DESIGN.md section 4): a bound of ONE row pair moves the odd rows of
    a call onto even positions of their launches.  At f64 the result is bit-equal all the same.  At f32 it may differ in the last bits,
    and only because the inner transforms do: RealFft.rfft of the same rows in another order shows the same dependence.  The handle may
    deviate exactly as far as RealFft does, and stays within its tolerance."""
    L, n = 1024, 300
    rng = np.random.default_rng(11)
    perm = [0, 3, 1, 4, 2, 5]
    for real in ("f64", "f32"):
        xh, yh = truth.rows(rng, 6, n, ndt(real)), truth.rows(rng, 6, n, ndt(real))
        x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
        whole, _ = make(fx, monkeypatch, False, n, L, -(n - 1), 2 * n - 1, real)
        per = 2 * (L // 2 + 1) * (8 if real == "f32" else 16) + 3 * L * (4 if real == "f32" else 8)
        monkeypatch.setenv("FOURIER_XCORR_SCRATCH_BYTES", str(per + 8))
        try:
            single, _ = make(fx, monkeypatch, False, n, L, -(n - 1), 2 * n - 1, real)
        finally:
            monkeypatch.delenv("FOURIER_XCORR_SCRATCH_BYTES")
        a, b = run(torch, whole, x, y), run(torch, single, x, y)
        rf = fx.RealFft(L, real, 0)
        z = torch.from_numpy(truth.rows(rng, 6, L, ndt(real))).cuda()
        inner_equal = torch.equal(rf.rfft(z)[perm], rf.rfft(z[perm].contiguous()))
        print(f"xcorr {real} one row pair a chunk: bit-equal {np.array_equal(a, b)}, max diff {np.abs(a - b).max():.3g};"
              f" RealFft.rfft on permuted rows bit-equal {inner_equal}")
        if real == "f64":
            assert inner_equal and np.array_equal(a, b)
        else:
            assert np.array_equal(a, b) or not inner_equal
        want = truth.full(xh, yh, L)
        note(real, "none", "composed chunks", "one row pair a chunk", truth.window_err(b, want, -(n - 1), 2 * n - 1), 4 * base(single, real))
