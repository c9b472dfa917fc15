"""Transforms along a strided axis on the MI355X: fourier_hip_transform_axis_* through Fft.transform_axis / transform_axis_ptr and
fourier_amd.fftn / fft2 on torch tensors, against numpy in f64 of the same input.  The CPU twin is tests/test_axis_emu.py (it covers
the forced transpose route, the chunk walks, the allocation-free property after reserve_axis and the error cases)."""
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


def want_axis(x, code, axis):
    n = x.shape[axis]
    f, i = np.fft.fft(x, axis=axis), None
    if code in (1, 2, 4):
        i = np.fft.ifft(x, axis=axis)
    return {0: f, 1: i, 2: i * n if i is not None else None, 3: f / np.sqrt(n), 4: i * np.sqrt(n) if i is not None else None}[code]


def want_fftn(x, code, dims):
    if code == 0:
        return np.fft.fftn(x, axes=dims)
    if code == 3:
        return np.fft.fftn(x, axes=dims, norm="ortho")
    if code == 1:
        return np.fft.ifftn(x, axes=dims)
    if code == 4:
        return np.fft.ifftn(x, axes=dims, norm="ortho")
    return np.fft.ifftn(x, axes=dims, norm="forward")  # unscaled inverse


def cplx(torch, shape, real, gen):
    dt = torch.complex64 if real == "f32" else torch.complex128
    return torch.randn(*shape, dtype=dt, device="cuda:0", generator=gen)


def tol(real, plan=None):
    blu = plan is not None and "bluestein" in plan.describe()
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-12)


# (N, inner, outer): lane, column-tile and transpose routes at GPU sizes
CASES = [(5, 4096, 3, "axis lane"), (17, 300, 2, "axis lane"), (31, 4096, 1, "axis lane"), (32, 7, 5, "axis lane"),
         (64, 32, 3, "axis column tile"), (256, 4096, 2, "axis column tile"), (2048, 4096, 1, "axis column tile"),
         (2048, 17, 2, "axis transpose"), (1000, 48, 3, "axis transpose"), (4096, 7, 2, "axis transpose"), (97, 2, 4, "axis transpose"),
         (243, 1, 3, "stockham")]


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_axis_routes_match_numpy_on_a_side_stream(torch, fa, real):
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    side = torch.cuda.Stream()
    for n, inner, outer, route in CASES:
        plan = (fa.create_fft_f32 if real == "f32" else fa.create_fft_f64)(n, 0)
        assert plan.describe_axis(inner).startswith(route), (n, inner, plan.describe_axis(inner))
        x = cplx(torch, (outer, n, inner), real, gen)
        xh = x.cpu().numpy().astype(np.complex128)
        codes = range(5) if n * inner * outer <= (1 << 21) else (0, 1)
        for code in codes:
            with torch.cuda.stream(side):
                y = torch.empty_like(x)
                plan.transform_axis(x, y, code, 1)
                z = x.clone()
                plan.transform_axis(z, z, code, -2)
            side.synchronize()
            w = want_axis(xh, code, 1)
            assert rel_l2(y.cpu().numpy(), w) <= tol(real, plan), (n, inner, outer, real, code)
            assert torch.equal(y, z), (n, inner, outer, real, code)  # in place = out of place, bit for bit


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fftn_and_fft2_match_numpy(torch, fa, real):
    gen = torch.Generator(device="cuda:0").manual_seed(12)
    for shape, dims in (((48, 64), None), ((3, 100, 16), (1, 2)), ((3, 100, 16), (-1, 0)), ((2, 5, 64, 17), None),
                        ((2, 5, 64, 17), (-3, -2)), ((4, 1, 33, 8), (1, 2, 3)), ((7, 2048), (0,))):
        x = cplx(torch, shape, real, gen)
        xh = x.cpu().numpy().astype(np.complex128)
        axes = tuple(range(len(shape))) if dims is None else tuple(d % len(shape) for d in dims)
        for code in range(5):
            y = fa.fftn(x, dims, code)
            assert rel_l2(y.cpu().numpy(), want_fftn(xh, code, axes)) <= 2 * tol(real), (shape, dims, code)
        z = x.clone()
        assert fa.fftn(z, dims, fa.Transform.Ifft, out=z) is z
        assert rel_l2(z.cpu().numpy(), want_fftn(xh, 1, axes)) <= 2 * tol(real), (shape, dims)
    x = cplx(torch, (3, 64, 100), real, gen)
    xh = x.cpu().numpy().astype(np.complex128)
    out = torch.empty_like(x)
    assert fa.fft2(x, out=out) is out
    assert rel_l2(out.cpu().numpy(), np.fft.fft2(xh)) <= 2 * tol(real)
    assert rel_l2(fa.fft2(x, fa.Transform.SqrtScaledIfft).cpu().numpy(), np.fft.ifft2(xh, norm="ortho")) <= 2 * tol(real)


def test_fftn_rejects_what_is_out_of_scope(torch, fa):
    x = torch.zeros(4, 8, dtype=torch.complex64, device="cuda:0")
    with pytest.raises(TypeError):
        fa.fftn(x.t())  # not contiguous
    with pytest.raises(TypeError):
        fa.fftn(np.zeros((4, 8), np.complex64))
    with pytest.raises(TypeError):
        fa.fftn(torch.zeros(4, 8, device="cuda:0"))  # real input


def test_column_tile_call_whose_block_exceeds_2_gib(torch, fa):
    n, inner = 2048, 1 << 18  # one block of 2^32 bytes in f32
    plan = fa.create_fft_f32(n, 0)
    assert plan.describe_axis(inner) == "axis column tile: L=2048"
    gen = torch.Generator(device="cuda:0").manual_seed(13)
    x = torch.randn(1, n, inner, dtype=torch.complex64, device="cuda:0", generator=gen)
    cols = torch.linspace(0, inner - 1, 64).long().to("cuda:0")
    before = x[0][:, cols].cpu().numpy().astype(np.complex128)
    plan.transform_axis(x, x, fa.Transform.Fft, 1)
    torch.cuda.synchronize()
    after = x[0][:, cols].cpu().numpy()
    del x
    assert rel_l2(after, np.fft.fft(before, axis=0)) <= 2e-6
