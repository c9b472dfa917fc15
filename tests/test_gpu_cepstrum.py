"""The cepstrum handle on the MI355X: fourier_hip_cepstrum_* through fourier_amd.Cepstrum on device buffers -- the cases of
tests/cepstrum_cases.py, which the CPU twin tests/test_cepstrum_emu.py runs on the emulator build (it also covers the argument checks of
the C ABI, the comparison with scipy and the allocation-free property after reserve) -- and real_cepstrum / minimum_phase on torch
tensors, 600 rows on both routes, and a captured graph replayed after its input was overwritten.  Against tests/cepstrum_truth.py (f64
numpy on the rounded inputs); measures and bounds (3 x base, 6 x base) are stated in tests/cepstrum_cases.py.  Every figure is printed
before it is asserted; the worst err / bound per (precision, mode, route) is printed at module end.  Every case runs once."""
import numpy as np
import pytest

import cepstrum_cases as cases
import cepstrum_truth as truth

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


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("i", range(5))
def test_one_launch(request, monkeypatch, real, mode, i):
    L, n, m = cases.ONE_LAUNCH[real][i]
    spilling = not cases.has_kernel(real, mode, L)  # f32 minimum phase at 2^15: an instance the product leaves out ...
    if spilling:
        monkeypatch.setenv(cases.SPILLING, "1")     # ... runs from the experiments library under its development switch
    cases.one_launch(request.getfixturevalue("bx" if spilling else "be"), real, mode, L, n, m, spilling)


def test_the_instances_left_out_of_the_product(be, bx, monkeypatch):
    """f32 minimum phase at 2^13 and 2^15: composed in the product; one launch and within the bound in the experiments library"""
    for L in (8192, 32768):
        plan, route = cases.make(be, L, L, L, "f32", truth.MINIMUM_PHASE, 1)
        assert route == "composed" and "no one-launch kernel" in plan.describe(), plan.describe()
    monkeypatch.setenv(cases.SPILLING, "1")
    cases.one_launch(bx, "f32", truth.MINIMUM_PHASE, 8192, 5000, 5000, True)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_composed(be, real, mode):
    for L in cases.COMPOSED:
        cases.composed(be, real, mode, L)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_routes_agree(be, real, mode):
    for L, n in ((2048, 1501), (4096, 2049)):
        cases.routes_agree(be, real, mode, L, n)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_known_answers(be, real, fusion):
    cases.known_answers(be, real, fusion)
    cases.magnitude_is_kept(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_floor_on_a_zero_row(be, real, fusion):
    cases.floor_on_a_zero_row(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_floor_whose_square_leaves_the_format(be, real, fusion):
    cases.floor_whose_square_leaves_the_format(be, real, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_zero_floor_on_a_zero_row_touches_nothing_else(be, real, fusion):
    for mode in cases.MODES:
        cases.zero_floor_on_a_zero_row(be, real, mode, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_log_mult(be, real, fusion):
    for mode in cases.MODES:
        cases.log_mult_half(be, real, mode, fusion)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_chunk_and_launch_walks(bx, monkeypatch, real, mode):
    cases.walks(bx, monkeypatch, real, mode)


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("mode", cases.MODES)
def test_more_workgroups_than_one_per_cu(be, real, mode):
    """600 rows at L = 2048 in one launch, against the truth and against the composed route within the two bounds"""
    L, n, batch = 2048, 1501, 600
    rng = np.random.default_rng(21)
    x = truth.rows(rng, batch, n, cases.ndt(real))
    cases.conditions(x, L)
    out, bnd = {}, 0.0
    for fusion in (1, 0):
        plan, route = cases.make(be, n, L, n, real, mode, fusion)
        assert route == ("one-launch" if fusion else "composed")
        out[route] = cases.check(be, plan, real, mode, route, x, L, f"L={L} n={n} batch={batch}")
        bnd += cases.bound(plan, real, mode)
    want = truth.full(mode, x, L)
    den = truth.kappa(x, L) * (np.linalg.norm(want, axis=-1) if mode == truth.MINIMUM_PHASE else 1.0)
    diff = float(np.max(np.linalg.norm(out["one-launch"].astype(np.float64) - out["composed"], axis=-1) / den))
    cases.note(real, mode, "routes", f"L={L} n={n} batch={batch}", diff, bnd)


# ---- the torch layer
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_real_cepstrum_and_minimum_phase_on_tensors(torch, fa, real):
    n, L = 1501, 2048
    rng = np.random.default_rng(31)
    xh = truth.rows(rng, 6, n, cases.ndt(real))
    cases.conditions(xh, L)
    cases.conditions(xh, L, 0.5)
    cases.conditions(xh, n)
    x = torch.from_numpy(xh.reshape(2, 3, n)).cuda()
    b = cases.base_of(real)
    for name, mode, f, kw, lm in (("real_cepstrum", truth.CEPSTRUM, fa.real_cepstrum, {}, 1.0),
                                  ("minimum_phase", truth.MINIMUM_PHASE, fa.minimum_phase, {}, 1.0),
                                  ("minimum_phase half", truth.MINIMUM_PHASE, fa.minimum_phase, {"half": True}, 0.5)):
        bnd = (3 if mode == truth.CEPSTRUM else 6) * b
        got = f(x, L, **kw)
        assert got.shape == x.shape and got.dtype == x.dtype
        cases.note(real, mode, "tensors", name, truth.err(mode, got.cpu().numpy().reshape(6, n), xh, L, n, lm), bnd)
        out = torch.empty_like(x)
        assert f(x, L, out=out, **kw) is out and torch.equal(out, got)
        few = f(x, L, 300, **kw)  # fewer outputs: the same values
        assert few.shape == (2, 3, 300)
        cases.note(real, mode, "tensors", name + " outputs=300", truth.err(mode, few.cpu().numpy().reshape(6, 300), xh, L, 300, lm), bnd)
        # length=None: L = n, an odd length on the composed route
        cases.note(real, mode, "tensors", name + " length=None", truth.err(mode, f(x, **kw).cpu().numpy().reshape(6, n), xh, n, n, lm), bnd)
        # a non-contiguous input is copied: a transposed view gives what its contiguous copy gives
        xt = x.transpose(0, 1)
        assert not xt.is_contiguous() and torch.equal(f(xt, L, **kw), f(xt.contiguous(), L, **kw))
        # in place
        y = x.clone()
        assert f(y, L, out=y, **kw) is y and torch.equal(y, got)
    floor = fa.real_cepstrum(torch.zeros(2, n, dtype=x.dtype, device="cuda"), L, log_floor=1e-3)
    assert abs(float(floor[0, 0]) - np.log(1e-3)) <= 3 * b * abs(np.log(1e-3)) and float(floor[:, 1:].abs().max()) <= 3 * b * abs(np.log(1e-3))
    # type, shape and device errors
    with pytest.raises(TypeError):
        fa.real_cepstrum(x.cpu(), L)
    with pytest.raises(TypeError):
        fa.minimum_phase(x.to(torch.complex64 if real == "f32" else torch.complex128), L)
    with pytest.raises(TypeError):
        fa.real_cepstrum(x.to(torch.float16), L)
    with pytest.raises(TypeError):
        fa.real_cepstrum(x, L, out=torch.empty(2, 3, n + 1, dtype=x.dtype, device="cuda"))
    with pytest.raises(TypeError):
        fa.minimum_phase(x, L, out=torch.empty(2, 3, n, dtype=torch.float64 if real == "f32" else torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        fa.minimum_phase(x, L, out=torch.empty(2, 3, n, dtype=x.dtype))
    with pytest.raises(ValueError):
        fa.real_cepstrum(x, n - 1)
    with pytest.raises(ValueError):
        fa.real_cepstrum(x, L, L + 1)
    with pytest.raises(ValueError):
        fa.minimum_phase(x, L, 0)
    with pytest.raises(ValueError):
        fa.real_cepstrum(x, L, 300, out=x.view(-1)[: 6 * 300].view(2, 3, 300))  # m != n: the output may not overlap the input
    plan = fa.Cepstrum(n, L, real, None, 0, 0)
    with pytest.raises(ValueError):
        plan.apply(x[..., :-1].contiguous())
    with pytest.raises(fa.FourierError):
        plan.apply(x, log_mult=0.0)


@pytest.mark.parametrize("mode", cases.MODES)
def test_a_captured_graph_reads_the_new_rows_at_replay(torch, fa, mode):
    """capture one call of Cepstrum.apply on the one-launch route, replay; overwrite the input buffer, replay again: the second
    output is the truth for the NEW rows"""
    L, n = 2048, 1501
    rng = np.random.default_rng(41)
    x1, x2 = truth.rows(rng, 6, n, np.float32), truth.rows(rng, 6, n, np.float32)
    cases.conditions(x2, L)
    plan, route = cases.make(cases.DeviceBackend(fa, torch), n, L, n, "f32", mode, 1)
    assert route == "one-launch"
    plan.reserve(6)
    x = torch.from_numpy(x1).cuda()
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan.apply(x, out=out)  # loads the kernels' code object (the first launch of a module is not capturable)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.apply(x, out=out)
    for which, xh in (("first", x1), ("new", x2)):
        x.copy_(torch.from_numpy(xh).cuda())
        graph.replay()
        torch.cuda.synchronize()
        cases.note("f32", mode, route, f"graph replay, the {which} rows", truth.err(mode, out.cpu().numpy(), xh, L, n), cases.bound(plan, "f32", mode))
