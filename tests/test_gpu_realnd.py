"""Real-input N-D transforms on the MI355X: fourier_amd.rfftn / irfftn / rfft2 / irfft2 (fourier_hip_realnd_*) on torch tensors,
against numpy in f64 of the same input.  The CPU twin is tests/test_realnd_emu.py (every code, rank 1 ... 4, odd and even W, the
chunk walks, the allocation-free property after reserve and the error cases)."""
import numpy as np
import pytest

from helpers import rel_l2

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


def tol(real, rank):
    return (2e-6 if rank <= 2 else 3e-6) if real == "f32" else 1e-12


@pytest.mark.parametrize("batch", [64, 96], ids=["one_chunk", "two_chunks"])
def test_rfft2_and_irfft2_of_2048_squares_f32(fa, torch, batch):
    g = torch.Generator(device="cuda").manual_seed(batch)
    x = torch.randn(batch, 2048, 2048, dtype=torch.float32, device="cuda", generator=g)
    X = fa.rfft2(x)
    assert X.shape == (batch, 2048, 1025) and X.dtype == torch.complex64
    xs, Xs = x[::16].cpu().numpy().astype(np.float64), X[::16].cpu().numpy()  # every 16th item: numpy f64 of the same input
    assert rel_l2(Xs, np.fft.rfft2(xs)) <= 2e-6
    y = fa.irfft2(X)
    assert rel_l2(y[::16].cpu().numpy(), xs) <= 2e-6
    Y = torch.complex(torch.randn(batch, 2048, 1025, device="cuda", generator=g), torch.randn(batch, 2048, 1025, device="cuda", generator=g))
    z = fa.irfft2(Y)  # not Hermitian: numpy's projection of columns 0 and W/2
    assert rel_l2(z[::16].cpu().numpy(), np.fft.irfft2(Y[::16].cpu().numpy().astype(np.complex128))) <= 2e-6


def test_describe_reports_packed_with_column_tiles_at_2048_squares(fa):
    for real in ("f32", "f64"):
        d = fa.RealFftN((2048, 2048), real, 0).describe()
        assert d.startswith("realnd packed: rows ") and "axis 0 (2048): axis column tile: L=2048" in d, d


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 64), (3, 96, 100, 128), (2, 37, 17, 30), (4, 5, 6, 7, 8), (2, 3, 4, 5, 6),
                                   (5, 33, 48, 1001), (3, 256, 255)])
def test_rfftn_and_irfftn_match_numpy(fa, torch, real, shape):
    rdt = torch.float32 if real == "f32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(len(shape) * 1000 + shape[-1])
    x = torch.randn(*shape, dtype=rdt, device="cuda", generator=g)
    rank = len(shape) - 1
    dims = tuple(range(1, len(shape)))
    xn = x.cpu().numpy().astype(np.float64)
    for code, norm in ((fa.Transform.Fft, "backward"), (fa.Transform.SqrtScaledFft, "ortho")):
        X = fa.rfftn(x, dims, code)
        assert rel_l2(X.cpu().numpy(), np.fft.rfftn(xn, axes=dims, norm=norm)) <= tol(real, rank), (shape, code)
    Y = torch.complex(torch.randn(X.shape, dtype=rdt, device="cuda", generator=g), torch.randn(X.shape, dtype=rdt, device="cuda", generator=g))
    Yn = Y.cpu().numpy().astype(np.complex128)
    for code, norm in ((fa.Transform.Ifft, "backward"), (fa.Transform.SqrtScaledIfft, "ortho"), (fa.Transform.UnscaledIfft, "forward")):
        y = fa.irfftn(Y, dims, shape[-1], code)
        assert y.dtype == rdt and tuple(y.shape) == shape
        assert rel_l2(y.cpu().numpy(), np.fft.irfftn(Yn, s=shape[1:], axes=dims, norm=norm)) <= tol(real, rank), (shape, code)
    assert rel_l2(fa.irfftn(fa.rfftn(x, dims), dims, shape[-1]).cpu().numpy(), xn) <= tol(real, rank)  # round trip


def test_dims_that_need_the_movedim_path_and_out(fa, torch):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(6, 40, 3, 32, dtype=torch.float64, device="cuda", generator=g)
    xn = x.cpu().numpy()
    for dims in ((1, 3), (3, 1), (0, 1, 3), (-1, -3), (2, 1)):
        X = fa.rfftn(x, dims)
        want = np.fft.rfftn(xn, axes=dims)
        assert X.shape == want.shape and rel_l2(X.cpu().numpy(), want) <= 1e-12, dims
        y = fa.irfftn(X, dims, x.shape[dims[-1]])
        assert rel_l2(y.cpu().numpy(), np.fft.irfftn(X.cpu().numpy(), s=[x.shape[d] for d in dims], axes=dims)) <= 1e-12, dims
        out = torch.empty(X.shape, dtype=X.dtype, device="cuda")
        assert fa.rfftn(x, dims, out=out) is out and torch.equal(out, X)
    out = torch.empty(6, 40, 3, 17, dtype=torch.complex128, device="cuda")
    with pytest.raises(TypeError):
        fa.rfftn(x, (1, 3), out=out[..., :16])  # not contiguous, wrong shape
    with pytest.raises(ValueError):
        fa.irfftn(out, (1, 3), 40)  # 17 half-spectrum values cannot hold a real length of 40


def test_odd_last_lengths_and_rank_one(fa, torch):
    g = torch.Generator(device="cuda").manual_seed(6)
    for shape in ((4, 63, 1001), (3, 5, 7, 9), (8, 4097), (5, 1, 3)):
        x = torch.randn(*shape, dtype=torch.float64, device="cuda", generator=g)
        dims = tuple(range(1, len(shape)))
        X = fa.rfftn(x, dims)
        assert rel_l2(X.cpu().numpy(), np.fft.rfftn(x.cpu().numpy(), axes=dims)) <= 1e-12, shape
        y = fa.irfftn(X, dims, shape[-1])
        assert rel_l2(y.cpu().numpy(), x.cpu().numpy()) <= 1e-12, shape
    x = torch.randn(7, 4096, dtype=torch.float32, device="cuda", generator=g)
    assert torch.equal(fa.rfftn(x, (-1,)), fa.create_rfft_f32(4096, 0).rfft(x))  # rank 1: the real plan's bits


def test_one_item_larger_than_2_gib(fa, torch):
    """f32 [16384, 32768]: 2 GiB of reals, a half spectrum of 2 GiB (mirror rows up to 2 GiB apart): Parseval, the DC term, sampled
    columns against a direct f64 evaluation, and the round trip."""
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(16384, 32768, dtype=torch.float32, device="cuda", generator=g)
    X = fa.rfft2(x)
    assert X.shape == (16384, 16385)
    n = x.numel()
    xs = x.double()
    e_x = float((xs ** 2).sum())
    a = X.abs().double() ** 2
    e_X = float(2 * a.sum() - a[:, 0].sum() - a[:, -1].sum()) / n  # Parseval over the half spectrum
    del a
    assert abs(e_X - e_x) <= 1e-5 * e_x
    assert abs(complex(X[0, 0]) - float(xs.sum())) <= 1e-5 * np.sqrt(n)
    m = torch.arange(32768, device="cuda", dtype=torch.float64)
    for k in (0, 1, 8191, 16384):  # column k = the FFT down the rows of each row's DFT at bin k
        ph = -2 * np.pi * k * m / 32768
        col = torch.fft.fft(torch.complex(xs @ torch.cos(ph), xs @ torch.sin(ph)), dim=0)
        assert rel_l2(X[:, k].cpu().numpy(), col.cpu().numpy()) <= 2e-6, k
    del xs
    y = fa.irfft2(X)
    assert float(((y - x).double() ** 2).sum()) <= (2e-6) ** 2 * e_x
