"""The MDCT handle on the MI355X: fourier_hip_mdct_* through the C ABI (Mdct.forward / inverse) and mdct / imdct on torch tensors,
against tests/mdct_truth.py (the dense cosine matrix in f64 numpy on the rounded input).  The CPU twin is tests/test_mdct_emu.py (it
also covers the argument checks, the chunk walks and the allocation-free property after reserve).

Tolerance, relative L2 over the whole output: forward twice tests/test_gpu_real.py's tol() for the inner plan's describe string (what
tests/test_gpu_r2r.py and tests/test_gpu_stft.py grant a plan plus twiddle sweeps), inverse and round trip twice that again."""
import numpy as np
import pytest

import mdct_truth as truth
from helpers import max_rel, rel_l2

pytestmark = pytest.mark.gpu

FUSED_N = (128, 256, 512, 1024, 2048)
SENTINEL = 77.0


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
    return fourier_amd


def tol(plan, real, inverse=False):
    blu = "bluestein" in plan.describe()
    base = (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)
    return (4 if inverse else 2) * base


def rdtype(torch, real):
    return torch.float32 if real == "f32" else torch.float64


def has_fused(real, n):
    return n in (128, 256, 512, 1024) or (n == 2048 and real == "f32")


def prefix(n, fused):
    if n % 2:
        return "mdct full-length, imdct full-length: "
    return "mdct fused rows, imdct composed: " if fused else "mdct composed, imdct composed: "


def check_forward(torch, fa, real, n, length, batch, center=True, window="default", normalized=False, offset=0):
    """both "fusion" values where the fused route exists, against the truth and each other; describe() says which route ran"""
    plan = fa.Mdct(n, real, center, 0)
    dt = rdtype(torch, real)
    g = torch.Generator(device="cuda").manual_seed(n + length + batch)
    w = None
    if window == "random":
        w = 0.5 + torch.rand(2 * n, dtype=dt, device="cuda", generator=g)
    plan.set_window(w)
    base = torch.randn(batch * length + offset, dtype=dt, device="cuda", generator=g)
    x = base[offset:].view(batch, length)
    assert plan.frames(length) == truth.frames(length, n, center) > 0
    npdt = np.float32 if real == "f32" else np.float64
    want = truth.mdct(x.cpu().numpy(), n, truth.sine_window(n, npdt) if w is None else w.cpu().numpy(), center, normalized)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        d = plan.describe()
        assert d.startswith(prefix(n, fusion == 1 and has_fused(real, n))), d
        got[fusion] = plan.forward(x, normalized).cpu().numpy()
        err, emax = rel_l2(got[fusion], want), max_rel(got[fusion], want)
        print(f"mdct {real} n={n} length={length} center={center} window={window} fusion={fusion}: err {err:.3g} tol {tol(plan, real):.3g} "
              f"max_rel {emax:.3g}")
        assert err <= tol(plan, real), (real, n, length, center, fusion, err, d)
        # the largest single error over the largest value, within twice the L2 bound (the ratio tests/test_gpu_parity.py grants,
        # tmax = 2 tl2): one wrong element among thousands hides in the L2 norm, not here
        assert emax <= 2 * tol(plan, real), (real, n, length, center, fusion, emax, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("real,n", [(real, n) for real in ("f32", "f64") for n in FUSED_N if has_fused(real, n)])
def test_fused_shapes(torch, fa, real, n):
    check_forward(torch, fa, real, n, 5 * n + 3, 3)                     # frames not a multiple of the tile, a workgroup spans two rows, a zero tail in the last two frames
    check_forward(torch, fa, real, n, 4 * n, 2, center=False)           # no padding path
    check_forward(torch, fa, real, n, 3 * n + 1, 2, offset=1)           # the input one element off its allocation
    check_forward(torch, fa, real, n, 4 * n, 2, window="random")        # an explicit window
    check_forward(torch, fa, real, n, 4 * n, 2)                         # the default sine window
    check_forward(torch, fa, real, n, 4 * n, 2, normalized=True)        # scaling
    check_forward(torch, fa, real, n, n // 2 + 1, 2)                    # a row shorter than one hop: every frame is an edge frame


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_and_full_length_shapes(torch, fa, real):
    for n, route in ((2, "mdct composed"), (6, "mdct composed"), (160, "mdct composed"), (960, "mdct composed"), (4096, "mdct composed"),
                     (1, "mdct full-length"), (5, "mdct full-length"), (255, "mdct full-length")):
        plan = check_forward(torch, fa, real, n, 5 * n + 3, 3, window="random")
        assert plan.describe().startswith(route), plan.describe()
        check_forward(torch, fa, real, n, 4 * n, 2, center=False)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_inverse_matches_the_truth_and_round_trips(torch, fa, real):
    g = torch.Generator(device="cuda").manual_seed(7)
    dt = rdtype(torch, real)
    for n in (256, 960, 255):
        for center in (True, False):
            plan = fa.Mdct(n, real, center, 0)
            length, batch = 5 * n + 3, 3
            x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
            X = plan.forward(x)  # the default sine window: Princen-Bradley
            nf = X.shape[1]
            back = min(length, plan.default_length(nf))
            y = plan.inverse(X, back).cpu().numpy()
            want = truth.imdct(X.cpu().numpy(), n, back, truth.sine_window(n, np.float32 if real == "f32" else np.float64), center)
            err = rel_l2(y, want)
            print(f"imdct {real} n={n} center={center}: err {err:.3g} tol {tol(plan, real, True):.3g}")
            assert err <= tol(plan, real, True), (real, n, center, err)  # against the truth everywhere
            # without padding only the samples two frames cover: n ... (frames - 1) n.  (The frames ignore what lies behind the last
            # whole hop, so for this length that is three samples short of length - n.)
            lo, hi = (0, back) if center else (n, (nf - 1) * n)
            xs = x.cpu().numpy()
            err = rel_l2(y[:, lo:hi], xs[:, lo:hi])
            print(f"round trip {real} n={n} center={center}: err {err:.3g} tol {tol(plan, real, True):.3g}")
            assert err <= tol(plan, real, True), (real, n, center, err)
            # a random window and `normalized`, against the truth
            w = 0.5 + torch.rand(2 * n, dtype=dt, device="cuda", generator=g)
            plan.set_window(w)
            Xr = torch.randn(batch, nf, n, dtype=dt, device="cuda", generator=g)
            y = plan.inverse(Xr, back - 5, True).cpu().numpy()
            want = truth.imdct(Xr.cpu().numpy(), n, back - 5, w.cpu().numpy(), center, True)
            err = rel_l2(y, want)
            print(f"imdct normalized {real} n={n} center={center}: err {err:.3g} tol {tol(plan, real, True):.3g}")
            assert err <= tol(plan, real, True), (real, n, center, err)


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    from fourier_amd import fft

    for dt, real in ((torch.float32, "f32"), (torch.float64, "f64")):
        n = 256
        x = torch.randn(2, 3, 2000, dtype=dt, device="cuda", generator=g)
        X = fa.mdct(x, n, normalized=True)
        nf = -(-2000 // n) + 1
        assert X.shape == (2, 3, nf, n) and X.dtype == dt and X.is_contiguous()  # leading dimensions fold into the batch
        want = truth.mdct(x.reshape(6, 2000).cpu().numpy(), n, truth.sine_window(n, np.float32 if real == "f32" else np.float64), True, True)
        base = 2e-6 if real == "f32" else 1e-13
        assert rel_l2(X.reshape(6, nf, n).cpu().numpy(), want) <= 2 * base
        y = fa.imdct(X, n, normalized=True, length=2000)
        assert y.shape == (2, 3, 2000) and y.dtype == dt
        assert rel_l2(y.cpu().numpy(), x.cpu().numpy()) <= 4 * base
        assert fa.imdct(X, n).shape == (2, 3, (nf - 1) * n)  # the default length
        assert fa.imdct(fa.mdct(x[0, 0, :1024], n, center=False), n, center=False).shape == (1024,)
        # one cached handle per (n, center, dtype, device)
        before = len(fft._PLANS)
        fa.mdct(x, n)
        fa.imdct(X, n)
        assert len(fft._PLANS) == before
        w = 0.5 + torch.rand(2 * n, dtype=dt, device="cuda", generator=g)
        Xw = fa.mdct(x, n, window=w)
        assert len(fft._PLANS) == before and not torch.equal(Xw, fa.mdct(x, n))  # the window is set on every call
        # out= on the handle
        plan = fa.Mdct(n, real, device=0)
        out = torch.empty(6, nf, n, dtype=dt, device="cuda")
        assert plan.forward(x.reshape(6, 2000), True, out=out) is out
        assert torch.equal(out, X.reshape(6, nf, n))
        back = torch.empty(6, 1900, dtype=dt, device="cuda")
        assert plan.inverse(out, 1900, True, out=back) is back and torch.equal(back.view(2, 3, 1900), y[..., :1900])
        with pytest.raises(TypeError):
            plan.forward(x.reshape(6, 2000), out=torch.empty(6, nf, n, dtype=dt))
        with pytest.raises(TypeError):
            plan.forward(x.reshape(6, 2000).to(torch.float64 if real == "f32" else torch.float32))
    x = torch.randn(4, 1000, device="cuda")
    with pytest.raises(TypeError):
        fa.mdct(x.cpu(), 256)
    with pytest.raises(TypeError):
        fa.mdct(x.to(torch.complex64), 256)
    with pytest.raises(TypeError):
        fa.mdct(x, 256, window=torch.ones(512, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        fa.mdct(x, 256, window=torch.ones(512))
    with pytest.raises(ValueError):
        fa.mdct(x, 256, window=torch.ones(511, device="cuda"))
    with pytest.raises(ValueError):
        fa.mdct(x, 0)
    with pytest.raises(ValueError):
        fa.mdct(x[:, :100], 256, center=False)
    with pytest.raises(TypeError):
        fa.imdct(x.to(torch.complex64), 256)
    with pytest.raises(ValueError):
        fa.imdct(torch.zeros(4, 9, 100, device="cuda"), 256)
    with pytest.raises(ValueError):
        fa.imdct(torch.zeros(4, 9, 256, device="cuda"), 256, length=8 * 256 + 1)


@pytest.mark.parametrize("n", [128, 256, 1024])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_output_on_an_odd_element(torch, fa, real, n):
    """The GPU twin of test_mdct_emu.py's test_input_and_output_offset_by_one_element: an output one element into its allocation is
    not aligned to a pair of reals, so the fused route stores single reals (a.pairs false) where it otherwise stores pairs.  Against the
    truth, bit-equal to the aligned output of the same route, the elements in front and behind untouched."""
    dt = rdtype(torch, real)
    g = torch.Generator(device="cuda").manual_seed(n)
    length, batch = 3 * n + 1, 2
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    plan = fa.Mdct(n, real, True, 0)
    nf = plan.frames(length)
    want = truth.mdct(x.cpu().numpy(), n, truth.sine_window(n, np.float32 if real == "f32" else np.float64))
    count = batch * nf * n
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        assert plan.describe().startswith(prefix(n, fusion == 1)), plan.describe()
        aligned = plan.forward(x)
        buf = torch.full((count + 2,), SENTINEL, dtype=dt, device="cuda")
        out = buf[1:1 + count].view(batch, nf, n)
        assert out.data_ptr() % (2 * out.element_size()) != 0
        assert plan.forward(x, out=out) is out
        err, emax = rel_l2(out.cpu().numpy(), want), max_rel(out.cpu().numpy(), want)
        print(f"mdct odd output {real} n={n} fusion={fusion}: err {err:.3g} max_rel {emax:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real) and emax <= 2 * tol(plan, real), (real, n, fusion, err, emax)
        assert buf[0].item() == SENTINEL and buf[-1].item() == SENTINEL, "an element beside the output was written"
        assert torch.equal(out, aligned), (real, n, fusion)


IMPULSE_N = [(128, 1), (128, 0), (256, 1), (256, 0), (6, 0), (250, 0), (255, 0)]


@pytest.mark.parametrize("n,fusion", IMPULSE_N)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_unit_impulses_give_one_column_of_the_cosine_matrix(torch, fa, real, n, fusion):
    """A known answer that one wrong element fails.  Every row is zero except for one unit sample; the sample sits at positions
    0, h-1, h, n-1, n, 3h-1, 3h, 2n-1 of an interior frame (both sides of the four branch boundaries of mdct_fold, where a random input
    averages a sign error into the L2 norm) and at the first and the last sample of the row (the zero-padded first and last frames).
    A frame that holds the sample at its position m is w[m] times row m of the cosine matrix; every other frame is exactly 0.0."""
    dt = rdtype(torch, real)
    g = torch.Generator(device="cuda").manual_seed(100 + n)
    h = n // 2
    length, f = 6 * n + 3, 3
    spots = [f * n - n + m for m in (0, h - 1, h, n - 1, n, 3 * h - 1, 3 * h, 2 * n - 1)] + [0, length - 1]
    x = torch.zeros(len(spots), length, dtype=dt, device="cuda")
    for row, t in enumerate(spots):
        x[row, t] = 1.0
    w = 0.5 + torch.rand(2 * n, dtype=dt, device="cuda", generator=g)
    plan = fa.Mdct(n, real, True, 0)
    plan.set_window(w)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith(prefix(n, fusion == 1)), plan.describe()
    nf = plan.frames(length)
    got = plan.forward(x).cpu().numpy()
    wh, C = w.cpu().numpy().astype(np.float64), truth.cosines(n)
    want = np.zeros((len(spots), nf, n))
    for row, t in enumerate(spots):
        for fr in range(nf):
            m = t + n - fr * n  # the sample's position in frame fr: the row starts n samples into the padded row
            if 0 <= m < 2 * n:
                want[row, fr] = wh[m] * C[m]
    assert np.array_equal(want, truth.mdct(x.cpu().numpy(), n, wh))  # the dense truth on these rows is that column, and exact zeros
    bound = 2 * tol(plan, real)
    worst = 0.0
    for row, t in enumerate(spots):
        zero = ~want[row].any(axis=1)
        assert zero.sum() == nf - 2 and np.all(got[row][zero] == 0.0), (real, n, fusion, t, "a frame without the sample is not zero")
        e = max_rel(got[row], want[row])
        worst = max(worst, e)
        assert e <= bound, (real, n, fusion, t, e, plan.describe())
    print(f"mdct impulses {real} n={n} fusion={fusion}: worst max_rel {worst:.3g} bound {bound:.3g}  [{plan.describe()}]")


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_round_trip_with_a_princen_bradley_window_other_than_the_sine(torch, fa, real):
    rng = np.random.default_rng(17)
    g = torch.Generator(device="cuda").manual_seed(17)
    dt = rdtype(torch, real)
    for n in (256, 250, 255):
        for center in (True, False):
            plan = fa.Mdct(n, real, center, 0)
            w = torch.from_numpy(truth.princen_bradley_window(rng, n, np.float32 if real == "f32" else np.float64)).cuda()
            plan.set_window(w)
            length, batch = 5 * n + 3, 3
            x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
            for fusion in (1, 0):
                plan.set_option("fusion", fusion)
                assert plan.describe().startswith(prefix(n, fusion == 1 and has_fused(real, n))), plan.describe()
                X = plan.forward(x)
                nf = X.shape[1]
                back = min(length, plan.default_length(nf))
                y = plan.inverse(X, back).cpu().numpy()
                lo, hi = (0, back) if center else (n, (nf - 1) * n)  # the span of test_inverse_matches_the_truth_and_round_trips
                err = rel_l2(y[:, lo:hi], x.cpu().numpy()[:, lo:hi])
                print(f"round trip, random Princen-Bradley window {real} n={n} center={center} fusion={fusion}: err {err:.3g} "
                      f"tol {tol(plan, real, True):.3g}")
                assert err <= tol(plan, real, True), (real, n, center, fusion, err)


@pytest.mark.parametrize("real,n", [(real, n) for real in ("f32", "f64") for n in FUSED_N if has_fused(real, n)])
def test_fused_forward_is_repeatable(torch, fa, real, n):
    """The same fused forward twenty times into fresh outputs: every result bit-equal to the first.  The kernel stages its outputs
    through LDS between barriers; a race there shows as a difference between runs."""
    g = torch.Generator(device="cuda").manual_seed(n)
    dt = rdtype(torch, real)
    length, batch = 5 * n + 3, 3
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    plan = fa.Mdct(n, real, True, 0)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("mdct fused rows"), plan.describe()
    nf = plan.frames(length)
    outs = [torch.full((batch, nf, n), float("nan"), dtype=dt, device="cuda") for _ in range(20)]
    for out in outs:
        plan.forward(x, out=out)
    torch.cuda.synchronize()
    err = rel_l2(outs[0].cpu().numpy(), truth.mdct(x.cpu().numpy(), n, truth.sine_window(n, np.float32 if real == "f32" else np.float64)))
    assert err <= tol(plan, real), (real, n, err)
    for i, out in enumerate(outs[1:]):
        assert torch.equal(out, outs[0]), (real, n, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """Forward and inverse captured on a side stream as the first calls of a handle that reserved (they must not allocate), replayed
    twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, length, batch = 256, 5 * 256 + 3, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randn(batch, length, dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    side = torch.cuda.Stream()
    other = fa.Mdct(n, "f32", True, 0)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.inverse(other.forward(xs[0]), length)
    side.synchronize()
    plan = fa.Mdct(n, "f32", True, 0)
    plan.set_option("fusion", fusion)
    assert plan.describe().startswith(prefix(n, fusion == 1)), plan.describe()
    plan.reserve(length, batch)
    nf = plan.frames(length)
    torch.cuda.synchronize()
    d = xs[0].clone()
    X = torch.empty(batch, nf, n, dtype=torch.float32, device="cuda")
    y = torch.empty(batch, length, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(d, out=X)  # the first calls on this plan: captured
        plan.inverse(X, length, out=y)
    w = truth.sine_window(n, np.float32)
    for x in xs[1:]:
        d.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eX = plan.forward(x)
        ey = plan.inverse(eX, length)
        torch.cuda.synchronize()
        assert torch.equal(X, eX) and torch.equal(y, ey), fusion
        assert rel_l2(X.cpu().numpy(), truth.mdct(x.cpu().numpy(), n, w)) <= tol(plan, "f32")
        assert rel_l2(y.cpu().numpy(), truth.imdct(X.cpu().numpy(), n, length, w)) <= tol(plan, "f32", True)
