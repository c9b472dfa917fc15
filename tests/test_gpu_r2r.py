"""DCT / DST of types II and III on the MI355X: fourier_hip_r2r_* through the C ABI (R2R.transform_batch_ptr) and dct / idct / dst /
idst on torch tensors, against the f64 definitions of tests/r2r_truth.py on the same (rounded) input.  The CPU twin is
tests/test_r2r_emu.py (it covers the argument checks, the chunk walk and the allocation-free property after reserve)."""
import numpy as np
import pytest

from helpers import rel_l2
from r2r_truth import KINDS, NORMS, want

pytestmark = pytest.mark.gpu


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


def tol(plan, real):
    """Twice test_gpu_real.py's tol() for the inner plan's describe string: what that file grants a two-stage composition."""
    blu = "bluestein" in plan.describe()
    return 2 * ((4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13))


def make(fa, n, real):
    return (fa.create_r2r_f32 if real == "f32" else fa.create_r2r_f64)(n, 0)


def rdtype(torch, real):
    return torch.float32 if real == "f32" else torch.float64


def check_length(torch, fa, n, real, batch, norms=("backward", "ortho"), seed=0):
    """Every kind through the raw-pointer ABI on the current stream, against the f64 definition of the same (rounded) input."""
    plan = make(fa, n, real)
    t = tol(plan, real)
    g = torch.Generator(device="cuda").manual_seed(seed + n)
    x = torch.randn(batch, n, dtype=rdtype(torch, real), device="cuda", generator=g)
    stream = torch.cuda.current_stream().cuda_stream
    cases = [(kind, norm) for kind in KINDS for norm in norms]
    y = [torch.empty_like(x) for _ in cases]  # one allocation each: every output aligned like a caller's
    for out, (kind, norm) in zip(y, cases):
        plan.transform_batch_ptr(x.data_ptr(), out.data_ptr(), batch, KINDS[kind], NORMS[norm], stream)
    yh, xh = torch.stack(y).cpu().numpy(), x.cpu().numpy()
    for i, (kind, norm) in enumerate(cases):
        idx, ref = want(kind, norm, xh)
        err = rel_l2(yh[i][:, idx], ref)
        assert err <= t, (n, real, kind, norm, err, plan.describe())


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_length_1_to_130_every_kind(torch, fa, real):
    for n in range(1, 131):
        check_length(torch, fa, n, real, batch=3)


@pytest.mark.parametrize("n", [1000, 1001, 4096, 4098, 1 << 16, 20014, 1 << 20])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_larger_lengths_and_batches_that_do_not_fill_the_last_wave(torch, fa, n, real):
    """h odd (4098), a large row (2^20), a Bluestein inner plan (20014 = 2 x 10007), odd N (1001)."""
    check_length(torch, fa, n, real, batch=3, norms=("backward",))
    check_length(torch, fa, n, real, batch=5, norms=("ortho",), seed=1)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_in_place_equals_out_of_place_and_round_trips(torch, fa, real):
    for n in (6, 7, 4096, 4098, 1001):
        plan = make(fa, n, real)
        x = torch.randn(5, n, dtype=rdtype(torch, real), device="cuda")
        for kind, inv in (("dct2", "dct3"), ("dst2", "dst3"), ("dct3", "dct2"), ("dst3", "dst2")):
            y = plan.transform(x, KINDS[kind], NORMS["ortho"])
            z = x.clone()
            assert plan.transform(z, KINDS[kind], NORMS["ortho"], out=z) is z
            assert torch.equal(y, z), (n, kind)
            back = plan.transform(y, KINDS[inv], NORMS["ortho"])
            assert rel_l2(back.cpu().numpy(), x.cpu().numpy()) <= 2 * tol(plan, real), (n, kind)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_torch_layer(torch, fa, real):
    dt = rdtype(torch, real)
    n = 96
    t = tol(make(fa, n, real), real)
    x = torch.randn(2, 3, n, dtype=dt, device="cuda")
    xh = x.cpu().numpy()
    for fn, kind in ((fa.dct, "dct"), (fa.dst, "dst")):
        for type in (2, 3):
            for norm in (None, "backward", "ortho", "forward"):
                y = fn(x, type=type, norm=norm)
                assert y.shape == x.shape and y.dtype == dt
                idx, ref = want(f"{kind}{type}", norm or "backward", xh)
                assert rel_l2(y.cpu().numpy()[..., idx], ref) <= t, (kind, type, norm)
    for fn, inv in ((fa.dct, fa.idct), (fa.dst, fa.idst)):
        for type in (2, 3):
            for norm in (None, "ortho", "forward"):
                back = inv(fn(x, type=type, norm=norm), type=type, norm=norm)
                assert rel_l2(back.cpu().numpy(), xh) <= 2 * t, (type, norm)
    # dim = 0 and a middle dim: moved last by a copy, moved back
    w = torch.randn(n, 5, dtype=dt, device="cuda")
    idx, ref = want("dct2", "backward", w.cpu().numpy().T)
    y = fa.dct(w, dim=0)
    assert y.shape == w.shape and y.is_contiguous()
    assert rel_l2(y.cpu().numpy().T[..., idx], ref) <= t
    m = torch.randn(2, n, 3, dtype=dt, device="cuda")
    idx, ref = want("dst3", "ortho", np.moveaxis(m.cpu().numpy(), 1, -1))
    assert rel_l2(np.moveaxis(fa.dst(m, type=3, norm="ortho", dim=1).cpu().numpy(), 1, -1)[..., idx], ref) <= t
    # out=, in place, a 1-D tensor
    out = torch.empty_like(x)
    assert fa.dct(x, out=out) is out and torch.equal(out, fa.dct(x))
    z = x.clone()
    assert fa.dct(z, out=z) is z and torch.equal(z, out)
    z0 = w.clone()
    assert fa.dct(z0, dim=0, out=z0) is z0 and torch.equal(z0, y)
    assert torch.equal(fa.dct(x[0, 0]), out[0, 0])
    assert torch.equal(x.cpu(), torch.from_numpy(xh)), "the input was modified"
    # errors
    for fn in (fa.dct, fa.idct, fa.dst, fa.idst):
        for type in (1, 4, 0):
            with pytest.raises(ValueError, match="1 and 4"):
                fn(x, type=type)
        with pytest.raises(ValueError):
            fn(x, norm="unitary")
        with pytest.raises(ValueError):
            fn(x, dim=3)
        with pytest.raises(TypeError):
            fn(x.to(torch.complex64))
        with pytest.raises(TypeError):
            fn(x.to(torch.float16))
        with pytest.raises(TypeError):
            fn(x.cpu())
        with pytest.raises(TypeError):
            fn(x, out=torch.empty(2, 3, n + 1, dtype=dt, device="cuda"))
        with pytest.raises(TypeError):
            fn(x, out=torch.empty(2, 3, n, dtype=torch.float16, device="cuda"))
        with pytest.raises(ValueError):
            fn(torch.zeros((), dtype=dt, device="cuda"))
    with pytest.raises(ValueError):
        make(fa, n, real).transform(torch.zeros(2, n + 1, dtype=dt, device="cuda"), 0)


def composition(torch, rplan, x):
    """The DCT-II a caller could write from RealFft.rfft and torch ops: index permutation, rfft, twiddle multiply, real part."""
    n = x.shape[-1]
    v = torch.cat([x[..., 0::2], x[..., 1::2].flip(-1)], dim=-1).contiguous()
    V = rplan.rfft(v)
    k = torch.arange(n // 2 + 1, device=x.device, dtype=torch.float64)
    c = torch.polar(torch.ones_like(k), -np.pi * k / (2 * n)).to(V.dtype)
    P = c * V
    y = torch.empty_like(x)
    y[..., : n // 2 + 1] = 2 * P.real
    y[..., n // 2 + 1:] = (-2 * P.imag[..., 1:(n + 1) // 2]).flip(-1)
    return y


@pytest.mark.parametrize("n", [4096, 1 << 18])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_equals_the_composition_from_rfft_and_torch_ops(torch, fa, n, real):
    plan = make(fa, n, real)
    rplan = (fa.create_rfft_f32 if real == "f32" else fa.create_rfft_f64)(n, 0)
    x = torch.randn(3, n, dtype=rdtype(torch, real), device="cuda")
    got = fa.dct(x)
    err = rel_l2(got.cpu().numpy(), composition(torch, rplan, x).cpu().numpy())
    assert err <= tol(plan, real), (n, real, err)
