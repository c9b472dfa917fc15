"""Convolution with a prepared filter bank on the MI355X: fourier_hip_conv_* through the C ABI (FftConv.apply_ptr /
set_filters_ptr), FftConv.apply and fftconv on torch tensors, against numpy in f64 on the same (rounded) inputs.  The CPU twin is
tests/test_conv_emu.py (argument checks, the chunk walk, the allocation-free property after reserve).

Tolerance, relative L2 over the whole output: three times tests/test_gpu_real.py's single-transform tolerance of the route (f32 2e-6,
4e-6 on a Bluestein plan; f64 1e-13, 1e-11), because three transforms in T contribute.
"""
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


def tol(plan, real):
    blu = "bluestein" in plan.describe()
    return 3 * ((4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13))


def dtype_of(torch, real, real_data):
    if real_data:
        return torch.float32 if real == "f32" else torch.float64
    return torch.complex64 if real == "f32" else torch.complex128


def want(x, h, correlate, first=0):
    """numpy in f64; row b with filter (first + b) mod F"""
    n = x.shape[-1]
    h = np.atleast_2d(h)
    hb = h[(first + np.arange(x.shape[0])) % h.shape[0]]
    if np.iscomplexobj(x):
        H = np.fft.fft(hb.astype(np.complex128), n, axis=-1)
        return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * (np.conj(H) if correlate else H), axis=-1)
    H = np.fft.rfft(hb.astype(np.float64), n, axis=-1)
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * (np.conj(H) if correlate else H), n=n, axis=-1)


def check(torch, fa, n, real, real_data, batch, F, taps, correlate=False, seed=0, describe=None, in_place=True):
    dt = dtype_of(torch, real, real_data)
    plan = fa.FftConv(n, real, real_data, 0)
    if describe is not None:
        assert plan.describe().startswith(describe), (n, real, real_data, plan.describe())
    t = tol(plan, real)
    g = torch.Generator(device="cuda").manual_seed(seed + n)
    x = torch.randn(batch, n, dtype=dt, device="cuda", generator=g)
    h = torch.randn(F, taps, dtype=dt, device="cuda", generator=g)
    stream = torch.cuda.current_stream().cuda_stream
    plan.set_filters_ptr(h.data_ptr(), taps, F, correlate, stream)
    assert plan.filters() == F
    y = torch.empty_like(x)
    plan.apply_ptr(x.data_ptr(), y.data_ptr(), batch, stream)
    xh, hh = x.cpu().numpy(), h.cpu().numpy()
    w = want(xh, hh, correlate)
    err = rel_l2(y.cpu().numpy(), w)
    assert err <= t, (n, real, real_data, batch, F, taps, correlate, err, plan.describe())
    assert np.array_equal(x.cpu().numpy(), xh) and np.array_equal(h.cpu().numpy(), hh), "apply modified its input or the taps"
    if in_place:
        plan.apply_ptr(x.data_ptr(), x.data_ptr(), batch, stream)
        err = rel_l2(x.cpu().numpy(), w)
        assert err <= t, ("in place", n, real, real_data, err, plan.describe())
    return plan


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_length_up_to_255(torch, fa, real, real_data):
    for n in range(1, 256):
        check(torch, fa, n, real, real_data, 3, 2, min(3, n), correlate=bool(n & 1), in_place=(n % 8 == 0))


def complex_class(real, k):
    top = 15 if real == "f32" else 14  # the longest one-launch two-level plan
    return "conv fused passes: " if k > top else "conv one-launch: " if k >= 11 else "conv composed: "


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_powers_of_two(torch, fa, real, real_data):
    for k in range(1, 23):
        n = 1 << k
        describe = "conv real fused untangle: " if real_data else complex_class(real, k)
        check(torch, fa, n, real, real_data, max(2, (1 << 21) // n), 3, min(n, 129), correlate=bool(k & 1), describe=describe,
              in_place=(k % 4 == 0))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_register_stages_mixed_tiles_and_bluestein_plans(torch, fa, real):
    for n in (1000, 5005, 44100, 999983, 1999966):
        check(torch, fa, n, real, False, 3, 2, 129, describe="conv composed: ")
        check(torch, fa, n, real, True, 3, 2, 129, correlate=True,
              describe="conv real fused untangle: " if n % 2 == 0 else "conv real composed: ")


def test_batches_and_filter_counts(torch, fa):
    for n, real_data in ((4096, False), (4096, True), (1 << 16, False), (1001, True), (100, False)):
        for batch, F in ((1, 1), (7, 1), (7, 7), (5, 9), (100, 64), (67, 3)):
            check(torch, fa, n, "f32", real_data, batch, F, 17, in_place=False)
    check(torch, fa, 8, "f64", True, 100003, 5, 3)      # a last wave that is not full
    # 64 rows per chunk of the scratch (two work arrays): a last chunk of 3, and 5 filters so that a chunk starts on every filter
    check(torch, fa, 1 << 20, "f32", False, 131, 5, 5, describe="conv fused passes: ")
    check(torch, fa, 1 << 20, "f32", False, 131, 64, 5, describe="conv fused passes: ")
    check(torch, fa, 1 << 14, "f32", False, 1003, 5, 5, describe="conv one-launch: ")
    check(torch, fa, 1 << 23, "f32", False, 2, 2, 5)   # beyond 2^22, whatever route the plan has
    check(torch, fa, 1 << 24, "f32", False, 2, 2, 5, describe="conv fused passes: ")  # three tile passes
    check(torch, fa, 1 << 20, "f32", True, 259, 64, 5, describe="conv real fused untangle: ")  # 255 rows per chunk: a last chunk of 4


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_routes_agree_with_the_composed_route(torch, fa, real):
    for n, real_data in ((1 << 12, False), (1 << 14, False), (1 << 16, False), (1 << 20, False), (1 << 20, True)):
        dt = dtype_of(torch, real, real_data)
        plan = fa.FftConv(n, real, real_data, 0)
        batch = max(3, (1 << 21) // n)
        g = torch.Generator(device="cuda").manual_seed(n)
        x = torch.randn(batch, n, dtype=dt, device="cuda", generator=g)
        h = torch.randn(2, 33, dtype=dt, device="cuda", generator=g)
        plan.set_filters(h)
        a = plan.apply(x)
        first = plan.describe()
        assert first.startswith("conv real fused untangle: " if real_data else complex_class(real, n.bit_length() - 1))
        plan.set_option("fusion", 0)
        assert plan.describe().startswith("conv real composed: " if real_data else "conv composed: ")
        b = plan.apply(x)
        w = want(x.cpu().numpy(), h.cpu().numpy(), False)
        t = tol(plan, real)
        ea, eb, eab = rel_l2(a.cpu().numpy(), w), rel_l2(b.cpu().numpy(), w), rel_l2(a.cpu().numpy(), b.cpu().numpy())
        assert ea <= t and eb <= t and eab <= t, (n, real, real_data, first, ea, eb, eab)


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
def test_headline_shape(torch, fa, real_data):
    n, batch = 1 << 20, 4096
    dt = dtype_of(torch, "f32", real_data)
    plan = fa.FftConv(n, "f32", real_data, 0)
    assert plan.describe().startswith("conv real fused untangle: " if real_data else "conv fused passes: ")
    t = tol(plan, "f32")
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(batch, n, dtype=dt, device="cuda", generator=g)
    y = torch.empty_like(x)
    # an impulse returns the input
    plan.set_filters(torch.ones(1, dtype=dt, device="cuda"))
    plan.apply(x, out=y)
    num = torch.linalg.vector_norm((y - x).reshape(-1)).item()
    den = torch.linalg.vector_norm(x.reshape(-1)).item()
    assert num / den <= t, ("impulse", num / den)
    # one filter for every row: sampled rows against numpy
    h = torch.randn(129, dtype=dt, device="cuda", generator=g)
    plan.set_filters(h)
    plan.apply(x, out=y)
    rows = [0, 1, 63, 64, 65, 254, 255, 256, 2047, 4094, 4095]  # both sides of the first chunk boundary (complex 64 rows, real 255), the last rows
    hh = h.cpu().numpy()
    err = rel_l2(y[rows].cpu().numpy(), want(x[rows].cpu().numpy(), hh, False))
    assert err <= t, ("sampled rows", err)
    # every row of a slice against the composed route
    lo, hi = 1000, 1300
    plan.set_option("fusion", 0)
    z = plan.apply(x[lo:hi])
    num = torch.linalg.vector_norm((z - y[lo:hi]).reshape(-1)).item()
    den = torch.linalg.vector_norm(z.reshape(-1)).item()
    assert num / den <= t, ("against composed", num / den)


def test_tensor_entry_points(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(11)
    for dt, real, real_data in ((torch.complex64, "f32", False), (torch.float64, "f64", True)):
        x = torch.randn(2, 3, 1000, dtype=dt, device="cuda", generator=g)
        h = torch.randn(3, 9, dtype=dt, device="cuda", generator=g)
        w = want(x.cpu().numpy().reshape(6, 1000), h.cpu().numpy(), False).reshape(2, 3, 1000)
        plan = fa.FftConv(1000, real, real_data)
        t = tol(plan, real)
        plan.set_filters(h)
        y = plan.apply(x)
        assert y.shape == x.shape and rel_l2(y.cpu().numpy(), w) <= t
        out = torch.empty_like(x)
        assert plan.apply(x, out=out) is out and rel_l2(out.cpu().numpy(), w) <= t
        z = x.clone()
        assert plan.apply(z, out=z) is z and rel_l2(z.cpu().numpy(), w) <= t
        assert rel_l2(fa.fftconv(x, h).cpu().numpy(), w) <= t
        wc = want(x.cpu().numpy().reshape(6, 1000), h[0].cpu().numpy(), True).reshape(2, 3, 1000)
        assert rel_l2(fa.fftconv(x, h[0].contiguous(), correlate=True).cpu().numpy(), wc) <= t  # the cached handle, a new bank
        z = x.clone()
        assert fa.fftconv(z, h, out=z) is z and rel_l2(z.cpu().numpy(), w) <= t
        with pytest.raises(TypeError):
            plan.apply(x.cpu())
        with pytest.raises(TypeError):
            plan.apply(x.to(torch.complex128 if not real_data else torch.float32))
        with pytest.raises(TypeError):
            plan.apply(x.transpose(0, 1))
        with pytest.raises(ValueError):
            plan.apply(x[..., :999].contiguous())
        with pytest.raises(TypeError):
            plan.apply(x, out=torch.empty(6, 1000, dtype=dt, device="cuda"))
        with pytest.raises(ValueError):
            plan.set_filters(torch.randn(1, 1001, dtype=torch.float64, device="cuda").to(dt))
        with pytest.raises(TypeError):
            plan.set_filters(h.cpu())
        with pytest.raises(TypeError):
            fa.fftconv(x.cpu(), h)


def test_graph_replay_of_apply_after_reserve(torch, fa):
    n, batch = 1 << 16, 8
    g = torch.Generator(device="cuda").manual_seed(12)
    x0 = torch.randn(batch, n, dtype=torch.complex64, device="cuda", generator=g)
    x1 = torch.randn(batch, n, dtype=torch.complex64, device="cuda", generator=g)
    h = torch.randn(3, 65, dtype=torch.complex64, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = fa.FftConv(n, "f32")  # loads the kernels' code object (the first launch of a module is not capturable)
    with torch.cuda.stream(side):
        other.set_filters(h)
        other.apply(x0)
    side.synchronize()
    plan = fa.FftConv(n, "f32")
    assert plan.describe().startswith("conv fused passes: ")
    plan.set_filters(h)
    plan.reserve(batch)
    torch.cuda.synchronize()
    d, o = x0.clone(), torch.empty_like(x0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.apply(d, out=o)  # the first apply on this plan: captured, must not allocate
    d.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    eager = plan.apply(x1)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), eager.cpu().numpy())
    assert rel_l2(o.cpu().numpy(), want(x1.cpu().numpy(), h.cpu().numpy(), False)) <= tol(plan, "f32")


def test_existing_transforms_are_untouched(fa):
    # Fft.describe() as the parent commit prints it
    assert fa.create_fft_f32(1 << 20, 0).describe() == DESCRIBE_2P20
    assert fa.create_fft_f32(999983, 0).describe() == DESCRIBE_999983
    assert fa.create_fft_f32(1 << 14, 0).describe() == DESCRIBE_2P14


DESCRIBE_2P20 = "stockham 1024x1024 f32"
DESCRIBE_999983 = "bluestein M=2097152 inner 2048x1024 f32"
DESCRIBE_2P14 = "stockham 128x128 one-launch f32"
