"""The delay handle on the MI355X: fourier_hip_delay_* through fourier_amd.Delay on device buffers -- the cases of tests/delay_cases.py,
which the CPU twin tests/test_delay_emu.py runs on the emulator build (it also covers the argument checks of the C ABI and the
allocation-free property after reserve) -- and fractional_delay / delay_and_sum on torch tensors, a captured graph whose delays change
between replays, and the pipeline gcc_phat -> argmax -> delay_and_sum without a host copy.  Against tests/delay_truth.py (f64 numpy on
the rounded inputs); measure and bound (3 x base) are stated in tests/delay_cases.py.  Every figure is printed before it is asserted;
the worst err / bound per (precision, route) is printed at module end.  Every case runs once."""
import numpy as np
import pytest

import delay_cases as cases
import delay_truth as truth

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
    yield fourier_amd
    cases.report("gpu")


@pytest.fixture(scope="module")
def be(torch, fa):
    return cases.DeviceBackend(fa, torch)


@pytest.fixture
def bx(torch, fa):
    """the backend bound to the experiments library for one test (tests/test_gpu_chunks.py): it reads the development switches from
    the environment at create.  A handle keeps the library it was created from."""
    import ctypes
    import os

    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield cases.DeviceBackend(fa, torch)
    _lib._lib = prev


def tdt(torch, real, cplx=False):
    return {("f32", False): torch.float32, ("f64", False): torch.float64, ("f32", True): torch.complex64, ("f64", True): torch.complex128}[(real, cplx)]


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("i", range(5))
def test_one_launch(be, real, i):
    L, n = cases.ONE_LAUNCH[real][i]
    cases.one_launch(be, real, L, n, weighted=i % 2 == 1)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
def test_composed(be, real, cplx, channels):
    for L in cases.COMPOSED:
        cases.composed(be, real, cplx, channels, L)


def test_huge_delays(be):
    cases.huge_delays(be)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_non_finite_delay_or_weight(be, real, fusion):
    cases.non_finite(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion,channels", [(1, 1), (0, 1), (0, 3)])
def test_repetition_and_power_of_two_scaling(be, real, fusion, channels):
    cases.repetition_and_scaling(be, real, fusion, channels)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_integer_delays_shift_and_zero_delay_is_the_input(be, real, fusion):
    cases.integer_delays_shift(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_chunk_and_launch_walks(bx, monkeypatch, real):
    cases.walks(bx, monkeypatch, real)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_more_workgroups_than_one_per_cu(be, real):
    """1025 rows at L = 2048 on both routes: every row against the truth"""
    L, n, batch = 2048, 1501, 1025
    rng = np.random.default_rng(21)
    x = truth.rows(rng, batch, n, cases.ndt(real))
    d = rng.uniform(-3000, 3000, batch).astype(cases.ndt(real))
    want = truth.delay(x, d, L)
    for fusion in (1, 0):
        plan, route = cases.make(be, n, L, real, fusion=fusion)
        cases.note(real, route, f"L={L} n={n} batch={batch}", truth.err(cases.run(be, plan, x, d), want, x), 3 * cases.base(plan, real))


# ---- the torch layer
@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
def test_fractional_delay_and_delay_and_sum_on_tensors(torch, fa, real, cplx):
    n, L = 600, 1000
    rng = np.random.default_rng(31)
    xh = truth.rows(rng, 6, n, cases.ndt(real, cplx)).reshape(2, 3, n)
    dh = np.array(truth.DELAYS, cases.ndt(real)).reshape(2, 3)
    wh = rng.uniform(0.5, 2.0, (2, 3)).astype(cases.ndt(real))
    x, d, w = (torch.from_numpy(a).cuda() for a in (xh, dh, wh))
    bound = 3 * (2e-6 if real == "f32" else 1e-13)
    flat = xh.reshape(6, n)
    for length in (None, L):
        want = truth.delay(flat, dh.ravel(), length or n)
        got = fa.fractional_delay(x, d, length)
        assert got.shape == x.shape and got.dtype == x.dtype
        cases.note(real, "tensors", f"fractional_delay length={length} complex={cplx}", truth.err(got.cpu().numpy().reshape(6, n), want, flat), bound)
        out = torch.empty_like(x)
        assert fa.fractional_delay(x, d, length, out=out) is out and torch.equal(out, got)
        want = truth.delay(flat, dh.ravel(), length or n, 3, wh.ravel())
        got = fa.delay_and_sum(x, d, w, length)
        assert got.shape == (2, n) and got.dtype == x.dtype
        cases.note(real, "tensors", f"delay_and_sum length={length} complex={cplx}", truth.err(got.cpu().numpy(), want, flat, 3, wh.ravel()), bound)
        out = torch.empty(2, n, dtype=x.dtype, device="cuda")
        assert fa.delay_and_sum(x, d, w, length, out=out) is out and torch.equal(out, got)
    # a Python number is broadcast on the device; delays of shape (3,) broadcast over the leading dimension; no weights: a plain sum
    got = fa.fractional_delay(x, 0.37, L)
    cases.note(real, "tensors", "a Python float", truth.err(got.cpu().numpy().reshape(6, n), truth.delay(flat, np.full(6, cases.ndt(real)(0.37)), L), flat), bound)
    got = fa.delay_and_sum(x, d[0], None, L)
    cases.note(real, "tensors", "broadcast delays", truth.err(got.cpu().numpy(), truth.delay(flat, np.tile(dh[0], 2), L, 3), flat, 3), bound)
    # in place for one channel
    y = x.clone()
    assert fa.fractional_delay(y, d, L, out=y) is y and torch.equal(y, fa.fractional_delay(x, d, L))
    # type, shape and device errors
    other = torch.float64 if real == "f32" else torch.float32
    with pytest.raises(TypeError):
        fa.fractional_delay(x.cpu(), d, L)
    with pytest.raises(TypeError):
        fa.fractional_delay(x, d.to(other), L)
    with pytest.raises(TypeError):
        fa.fractional_delay(x, d.cpu(), L)
    with pytest.raises(TypeError):
        fa.delay_and_sum(x, d, w.to(other), L)
    with pytest.raises(TypeError):
        fa.fractional_delay(x, "1.0", L)
    with pytest.raises(TypeError):
        fa.fractional_delay(x, d, L, out=torch.empty(2, 3, n + 1, dtype=x.dtype, device="cuda"))
    with pytest.raises(TypeError):
        fa.delay_and_sum(x, d, w, L, out=torch.empty(2, 3, n, dtype=x.dtype, device="cuda"))
    with pytest.raises(ValueError):
        fa.fractional_delay(x, torch.zeros(4, dtype=d.dtype, device="cuda"), L)
    with pytest.raises(ValueError):
        fa.fractional_delay(x, d, n - 1)
    with pytest.raises(ValueError):
        fa.delay_and_sum(x[0, 0], d[0, 0], None, L)
    with pytest.raises(ValueError):
        fa.delay_and_sum(x, d, w, L, out=x.view(-1)[: 2 * n].view(2, n))  # C > 1: the output may not overlap the input
    plan = fa.Delay(n, L, real, not cplx, 3, 0)
    with pytest.raises(ValueError):
        plan.apply(x.view(6, n)[:4], d.view(-1)[:4])  # 4 rows, 3 channels
    with pytest.raises(ValueError):
        plan.apply(x.view(6, n), d.view(-1)[:3])


@pytest.mark.parametrize("fusion", [1, 0])
def test_a_captured_graph_reads_the_delays_at_replay(torch, fa, fusion):
    """reserve, capture one call, replay; overwrite the delays tensor on the device, replay again: the second output is the truth for
    the NEW delays"""
    L, n = 2048, 1501
    rng = np.random.default_rng(41)
    xh = truth.rows(rng, 6, n, np.float32)
    d1 = np.array(truth.DELAYS, np.float32)
    d2 = np.array(truth.DELAYS[::-1], np.float32) * np.float32(1.5)
    plan, route = cases.make(cases.DeviceBackend(fa, torch), n, L, "f32", fusion=fusion)
    plan.reserve(6)
    x, d = torch.from_numpy(xh).cuda(), torch.from_numpy(d1).cuda()
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan.apply(x, d, out=out)  # loads the kernels' code object (the first launch of a module is not capturable)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.apply(x, d, out=out)
    for which, dh in (("first", d1), ("new", d2)):
        d.copy_(torch.from_numpy(dh).cuda())
        graph.replay()
        torch.cuda.synchronize()
        cases.note("f32", route, f"graph replay, the {which} delays", truth.err(out.cpu().numpy(), truth.delay(xh, dh, L), xh), 3 * 2e-6)


def test_gcc_phat_argmax_feeds_delay_and_sum_without_a_host_copy(torch, fa):
    """three noisy copies of a spike row at integer lags: gcc_phat against the first, argmax on the device, the negated lags into
    delay_and_sum; checked against the truth for those lags, and the lags are the ones put in"""
    n, lags = 1024, (0, 5, 17)
    rng = np.random.default_rng(51)
    sigma = 0.1 / np.sqrt(n)
    clean = sigma * rng.standard_normal(n)
    clean[n // 3] += 1.0
    xh = np.zeros((3, n))
    for c, lag in enumerate(lags):
        xh[c, lag:] = clean[:n - lag]
    xh = (xh + sigma * rng.standard_normal((3, n))).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    max_lag = 32
    r = fa.gcc_phat(x[:1].expand(3, n).contiguous(), x, max_lag)  # the peak is at the lag by which a channel trails the first
    found = (torch.argmax(r, dim=-1) - max_lag).to(torch.float32)  # stays on the device
    got = fa.delay_and_sum(x, -found, None, 2 * n)
    assert got.shape == (n,)
    assert found.cpu().tolist() == [float(v) for v in lags]
    want = truth.delay(xh, -np.array(lags, np.float32), 2 * n, 3)
    cases.note("f32", "pipeline", "gcc_phat -> argmax -> delay_and_sum", truth.err(got.cpu().numpy()[None, :], want, xh, 3), 3 * 2e-6)
    assert int(np.argmax(got.cpu().numpy())) == n // 3 and got.cpu().numpy()[n // 3] > 2.5  # the three spikes add up
