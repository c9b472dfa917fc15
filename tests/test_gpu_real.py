"""Real-input transforms on the MI355X: fourier_hip_real_* through the C ABI (RealFft.forward_batch_ptr / inverse_batch_ptr) and
RealFft.rfft / irfft on torch tensors, against numpy's rfft / irfft in f64 of the same input.  The CPU twin is
tests/test_real_emu.py (it covers the allocation-free property after reserve; no HIP graph is captured here)."""
import numpy as np
import pytest

from helpers import rel_l2

pytestmark = pytest.mark.gpu

CODES_FWD = (0, 3)
CODES_INV = (1, 2, 4)


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
    blu = "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def make(fa, n, real):
    return (fa.create_rfft_f32 if real == "f32" else fa.create_rfft_f64)(n, 0)


def dtypes(torch, real):
    return (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)


def want_forward(x, code):
    y = np.fft.rfft(np.asarray(x, np.float64), axis=-1)
    return y / np.sqrt(x.shape[-1]) if code == 3 else y


def want_inverse(X, n, code):
    y = np.fft.irfft(np.asarray(X, np.complex128), n=n, axis=-1)
    return {1: y, 2: n * y, 4: np.sqrt(n) * y}[code]


def check_length(torch, fa, n, real, batch, codes_fwd=CODES_FWD, codes_inv=CODES_INV, seed=0):
    """Every code through the raw-pointer ABI on the current stream, against numpy f64 of the same (rounded) input."""
    rdt, cdt = dtypes(torch, real)
    plan = make(fa, n, real)
    t = tol(plan, real)
    g = torch.Generator(device="cuda").manual_seed(seed + n)
    x = torch.randn(batch, n, dtype=rdt, device="cuda", generator=g)
    X = torch.randn(batch, n // 2 + 1, dtype=cdt, device="cuda", generator=g)
    stream = torch.cuda.current_stream().cuda_stream
    xh, Xh = x.cpu().numpy(), X.cpu().numpy()
    for code in codes_fwd:
        y = torch.empty(batch, n // 2 + 1, dtype=cdt, device="cuda")
        plan.forward_batch_ptr(x.data_ptr(), y.data_ptr(), batch, code, stream)
        err = rel_l2(y.cpu().numpy(), want_forward(xh, code))
        assert err <= t, (n, real, code, err, plan.describe())
    for code in codes_inv:
        y = torch.empty(batch, n, dtype=rdt, device="cuda")
        plan.inverse_batch_ptr(X.data_ptr(), y.data_ptr(), batch, code, stream)
        err = rel_l2(y.cpu().numpy(), want_inverse(Xh, n, code))
        assert err <= t, (n, real, code, err, plan.describe())
    assert np.array_equal(X.cpu().numpy(), Xh), "the inverse modified its input"


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_length_1_to_255_every_code(torch, fa, real):
    for n in range(1, 256):
        check_length(torch, fa, n, real, batch=3)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_powers_of_two_2_to_2_24(torch, fa, real):
    for k in range(1, 25):
        n = 1 << k
        check_length(torch, fa, n, real, batch=max(1, (1 << 21) // n), codes_fwd=(0, 3), codes_inv=(1, 4))


@pytest.mark.parametrize("n", [10010, 1999966, 999983])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_register_stage_bluestein_and_odd_inner_plans(torch, fa, n, real):
    check_length(torch, fa, n, real, batch=2, codes_fwd=(0, 3), codes_inv=(1, 2))


@pytest.mark.parametrize("n,batch", [(1000, 5), (1 << 16, 3), (4097, 3), (1 << 20, 3)])
def test_batches_that_do_not_fill_the_last_wave(torch, fa, n, batch):
    check_length(torch, fa, n, "f32", batch=batch, codes_fwd=(0,), codes_inv=(1,))


@pytest.mark.parametrize("n", [2, 64, 1000, 1001, 4096, 1 << 18, 999983])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_forward_equals_the_complex_transform_of_the_widened_input(torch, fa, n, real):
    rdt, cdt = dtypes(torch, real)
    plan = make(fa, n, real)
    cplan = (fa.create_fft_f32 if real == "f32" else fa.create_fft_f64)(n, 0)
    x = torch.randn(3, n, dtype=rdt, device="cuda")
    full = torch.empty(3, n, dtype=cdt, device="cuda")
    cplan.transform(x.to(cdt), full, fa.Transform.Fft)
    half = plan.rfft(x)
    err = rel_l2(half.cpu().numpy(), full[:, : n // 2 + 1].cpu().numpy())
    assert err <= 2 * tol(plan, real) + 2 * (4e-6 if real == "f32" else 1e-11) * ("bluestein" in cplan.describe()), (n, real, err)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_torch_rfft_irfft_on_leading_dimensions(torch, fa, real):
    rdt, cdt = dtypes(torch, real)
    n = 1 << 12
    plan = make(fa, n, real)
    x = torch.randn(2, 3, n, dtype=rdt, device="cuda")
    X = plan.rfft(x)
    assert X.shape == (2, 3, n // 2 + 1) and X.dtype == cdt
    assert rel_l2(X.cpu().numpy(), want_forward(x.cpu().numpy(), 0)) <= tol(plan, real)
    Xs = plan.rfft(x, fa.Transform.SqrtScaledFft)
    assert rel_l2(Xs.cpu().numpy(), want_forward(x.cpu().numpy(), 3)) <= tol(plan, real)
    back = plan.irfft(X)
    assert back.shape == (2, 3, n) and back.dtype == rdt
    assert rel_l2(back.cpu().numpy(), x.cpu().numpy()) <= 2 * tol(plan, real)
    with pytest.raises(TypeError):
        plan.rfft(x.to(cdt))
    with pytest.raises(ValueError):
        plan.irfft(X[..., :-1].contiguous())


def test_c2_shape_round_trip_and_parseval_against_the_complex_plan(torch, fa):
    """f32 N = 2^20, batch 4096 (the headline C2 shape): sampled rows against numpy, every row's round trip and energy (Parseval),
    and a slice of rows against the library's complex plan of the same N."""
    n, batch = 1 << 20, 4096
    plan = fa.create_rfft_f32(n, 0)
    x = torch.randn(batch, n, dtype=torch.float32, device="cuda")
    X = plan.rfft(x)
    back = plan.irfft(X)
    torch.cuda.synchronize()
    rows = [0, 1, 2047, 4095]
    xs = x[rows].cpu().numpy()
    assert rel_l2(X[rows].cpu().numpy(), want_forward(xs, 0)) <= 2e-6
    assert rel_l2(back[rows].cpu().numpy(), xs) <= 4e-6
    err = ((back - x).double().pow(2).sum(dim=1) / x.double().pow(2).sum(dim=1)).sqrt().max().item()
    assert err <= 4e-6, err
    e_time = x.double().pow(2).sum(dim=1)
    mag = X.abs().double().pow(2)
    e_freq = (2 * mag.sum(dim=1) - mag[:, 0] - mag[:, -1]) / n
    assert ((e_freq - e_time).abs() / e_time).max().item() <= 1e-5
    del back, mag
    cplan = fa.create_fft_f32(n, 0)
    sl = x[:64].to(torch.complex64)
    full = torch.empty_like(sl)
    cplan.transform(sl, full, fa.Transform.Fft)
    assert rel_l2(X[:64].cpu().numpy(), full[:, : n // 2 + 1].cpu().numpy()) <= 4e-6
