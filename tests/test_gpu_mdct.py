"""The MDCT handle on the MI355X: fourier_hip_mdct_* through the C ABI (Mdct.forward / inverse) and mdct / imdct on torch tensors,
against tests/mdct_truth.py (the dense cosine matrix in f64 numpy on the rounded input).  The CPU twin is tests/test_mdct_emu.py (it
also covers the argument checks, the chunk walks and the allocation-free property after reserve).

Tolerance, relative L2 over the whole output: forward twice tests/test_gpu_real.py's tol() for the inner plan's describe string (what
tests/test_gpu_r2r.py and tests/test_gpu_stft.py grant a plan plus twiddle sweeps), inverse and round trip twice that again."""
import numpy as np
import pytest

import mdct_truth as truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

FUSED_N = (128, 256, 512, 1024, 2048)


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
        err = rel_l2(got[fusion], want)
        print(f"mdct {real} n={n} length={length} center={center} window={window} fusion={fusion}: err {err:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real), (real, n, length, center, fusion, err, d)
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
