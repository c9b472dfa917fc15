"""The polyphase synthesis bank handle on the MI355X: fourier_hip_ipfb_* through the C ABI (Ipfb.inverse_ptr) and pfb_synthesize on torch
tensors, against tests/ipfb_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_ipfb_emu.py (it also covers the
argument checks, length(), the allocation-free property after reserve and pfb_reconstruction_terms).

Every call goes into an output between guard elements prefilled with a sentinel, and the input is compared afterwards with a clone.

Tolerance, relative L2 over the whole output: the analysis tests' figure for a transform plus one more rounding stage, twice
tests/test_gpu_real.py's tol() for the inner plan's describe string: 2 x (2e-6 f32, 1e-13 f64; Bluestein inner plans 4e-6 / 1e-11);
tests/test_ipfb_emu.py shows the overlap sum's share of it.  The largest single error, over the largest value, stays within twice
that.  A round trip through both handles gets the sum of the two handles' tolerances."""
import ctypes
import os

import numpy as np
import pytest

import ipfb_truth as truth
from helpers import max_rel, rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
GUARD = 64
KINDS = [("f32", False), ("f32", True), ("f64", False), ("f64", True)]


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
    return 2 * ((4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13))


def dtypes(torch, real):
    return (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)


def bins_of(P, real_output):
    return P // 2 + 1 if real_output else P


def spectrum(torch, g, real, shape):
    rt = dtypes(torch, real)[0]
    return torch.view_as_complex(torch.randn(*shape, 2, dtype=rt, device="cuda", generator=g))


def signal(torch, g, real, real_rows, shape):
    rt = dtypes(torch, real)[0]
    if real_rows:
        return torch.randn(*shape, dtype=rt, device="cuda", generator=g)
    return torch.view_as_complex(torch.randn(*shape, 2, dtype=rt, device="cuda", generator=g))


def filter_of(torch, fa, g, real, P, T, prototype=False):
    rt = dtypes(torch, real)[0]
    if prototype:
        return fa.pfb_prototype(P, T, rt).cuda()
    return 0.5 + torch.rand(P * T, dtype=rt, device="cuda", generator=g)


def bits(torch, t):
    return torch.view_as_real(t) if t.is_complex() else t


def inverse(torch, plan, Y, length, offset=0):
    """inverse_ptr into a buffer between guard elements (the output `offset` elements further on); checks the guards and that the input
    is unmodified"""
    rt, ct = dtypes(torch, plan.real)
    batch, nf, _ = Y.shape
    before = Y.clone()
    buf = torch.full((batch * length + 2 * GUARD + offset,), SENTINEL, dtype=rt if plan.real_output else ct, device="cuda")
    lo, hi = GUARD + offset, GUARD + offset + batch * length
    plan.inverse_ptr(Y.data_ptr(), buf[lo:].data_ptr(), nf, length, batch, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all()), "a guard element was written"
    assert torch.equal(torch.view_as_real(Y), torch.view_as_real(before)), "inverse modified its input"
    return buf[lo:hi].view(batch, length).clone()


def check(torch, fa, real, real_output, P, T, D, nf, batch, cuts=(0,), use_filter=True, prototype=False, offset=0):
    """length = full(frames) - cut for every cut, against the truth; returns the last result too"""
    plan = fa.Ipfb(P, T, real, D, real_output, 0)
    d = plan.describe()
    assert d.startswith("ipfb composed: "), d
    g = torch.Generator(device="cuda").manual_seed(7 * P + T + D + nf)
    h = filter_of(torch, fa, g, real, P, T, prototype) if use_filter else None
    plan.set_filter(h)
    Y = spectrum(torch, g, real, (batch, nf, bins_of(P, real_output)))
    full = truth.full(nf, P, T, D)
    assert plan.length(nf) == full and plan.bins() == bins_of(P, real_output)
    hh = None if h is None else h.cpu().numpy()
    for cut in cuts:
        want = truth.synth(Y.cpu().numpy(), hh, P, T, D, real_output, full - cut)
        y = inverse(torch, plan, Y, full - cut, offset)
        got = y.cpu().numpy()
        err, emax = rel_l2(got, want), max_rel(got, want)
        print(f"ipfb {real} {'real' if real_output else 'complex'} P={P} T={T} D={D} frames={nf} length={full - cut} offset={offset}: "
              f"err {err:.3g} tol {tol(plan, real):.3g} max_rel {emax:.3g}  [{d}]")
        assert err <= tol(plan, real), (real, real_output, P, T, D, nf, cut, err, d)
        assert emax <= 2 * tol(plan, real), (real, real_output, P, T, D, nf, cut, emax, d)
    return plan, y


@pytest.mark.parametrize("real,real_output", KINDS)
def test_shapes(torch, fa, real, real_output):
    P = 256
    check(torch, fa, real, real_output, P, 4, P, 9, 3, cuts=(0, 5))           # (a) critically sampled; a shortened, odd row
    check(torch, fa, real, real_output, P, 3, 37, 5, 2, cuts=(0, 1))          # (b) cover 21; odd rows: the single-real store runs
    check(torch, fa, real, real_output, P, 16, 192, 30, 2, prototype=True)    # (c) oversampled prototype, cover 22
    check(torch, fa, real, real_output, P, 4, P, 9, 3, use_filter=False)      # (e) the default filter of ones
    check(torch, fa, real, real_output, P, 3, 64, 6, 2, cuts=(0, 3), offset=1)  # (f) the output one element off an allocation


@pytest.mark.parametrize("real,real_output", KINDS)
def test_gaps_are_exact_zeros(torch, fa, real, real_output):
    """(d) D = P T + 8: the 8 samples between two frames are covered by none, and are zeros where the sentinel was"""
    P, T = 256, 2
    D = P * T + 8
    _, y = check(torch, fa, real, real_output, P, T, D, 3, 2)
    for f in range(2):
        gap = y[:, f * D + P * T: (f + 1) * D]
        assert gap.shape[1] == 8 and bool((gap == 0).all()), gap
    assert bool((y[:, : P * T] != 0).all())


@pytest.mark.parametrize("real,real_output", KINDS)
def test_set_filter_null_restores_the_ones(torch, fa, real, real_output):
    """(e)"""
    P, T, D, nf = 256, 2, 192, 4
    g = torch.Generator(device="cuda").manual_seed(9)
    plan = fa.Ipfb(P, T, real, D, real_output, 0)
    Y = spectrum(torch, g, real, (1, nf, plan.bins()))
    h = filter_of(torch, fa, g, real, P, T)
    ones = plan.inverse(Y)
    plan.set_filter(h)
    with_h = plan.inverse(Y)
    assert rel_l2(with_h.cpu().numpy(), truth.synth(Y.cpu().numpy(), h.cpu().numpy(), P, T, D, real_output)) <= tol(plan, real)
    plan.set_filter(None)
    again = plan.inverse(Y)
    assert torch.equal(bits(torch, again), bits(torch, ones)) and not torch.equal(bits(torch, with_h), bits(torch, ones))
    assert rel_l2(ones.cpu().numpy(), truth.synth(Y.cpu().numpy(), None, P, T, D, real_output)) <= tol(plan, real)


@pytest.mark.parametrize("real,real_output", KINDS)
def test_other_inner_plans(torch, fa, real, real_output):
    """(g) mixed radix, a multi-pass length, and the full-length real route"""
    for P in (400, 4096):
        plan, _ = check(torch, fa, real, real_output, P, 2, 3 * P // 4, 3, 2, cuts=(0, 7))
        assert "stockham" in plan.describe(), plan.describe()
    if real_output:
        plan, _ = check(torch, fa, real, True, 63, 3, 40, 5, 2, cuts=(0, 1))
        assert plan.describe().startswith("ipfb composed: real full-length: "), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("real_rows", [True, False])
def test_round_trips_with_the_analysis_handle(torch, fa, real, real_rows):
    """(h) the two exact pairs of include/fourier.h, through fourier_amd.Pfb on the same device"""
    rt = dtypes(torch, real)[0]
    g = torch.Generator(device="cuda").manual_seed(11)
    P, batch = 256, 2
    # T = 1, D = P / 2, h = g = the periodic sqrt-Hann window: the interior, where two frames cover every sample
    D, nf = P // 2, 7
    length = P + (nf - 1) * D
    x = signal(torch, g, real, real_rows, (batch, length))
    w = torch.sqrt(0.5 - 0.5 * torch.cos(2 * np.pi * torch.arange(P, dtype=torch.float64) / P)).to(rt).cuda()
    ana, syn = fa.Pfb(P, 1, real, D, real_rows, 0), fa.Ipfb(P, 1, real, D, real_rows, 0)
    ana.set_filter(w)
    syn.set_filter(w)
    y = inverse(torch, syn, ana.forward(x), length)
    err = rel_l2(y[:, D: nf * D].cpu().numpy(), x[:, D: nf * D].cpu().numpy())
    print(f"ipfb round trip sqrt-Hann {real} {'real' if real_rows else 'complex'}: err {err:.3g} tol {tol(ana, real) + tol(syn, real):.3g}")
    assert err <= tol(ana, real) + tol(syn, real)
    # T = 4, D = P, h = g = ones on the first P coefficients: the first frames * P samples come back, the rest is zero
    T, nf = 4, 5
    length = P * T + (nf - 1) * P
    x = signal(torch, g, real, real_rows, (batch, length))
    w = torch.zeros(P * T, dtype=rt, device="cuda")
    w[:P] = 1
    ana, syn = fa.Pfb(P, T, real, P, real_rows, 0), fa.Ipfb(P, T, real, P, real_rows, 0)
    ana.set_filter(w)
    syn.set_filter(w)
    assert ana.frames(length) == nf and syn.length(nf) == length
    y = inverse(torch, syn, ana.forward(x), length)
    err = rel_l2(y[:, : nf * P].cpu().numpy(), x[:, : nf * P].cpu().numpy())
    print(f"ipfb round trip first-block ones {real} {'real' if real_rows else 'complex'}: err {err:.3g}")
    assert err <= tol(ana, real) + tol(syn, real)
    assert bool((y[:, nf * P:] == 0).all())


@pytest.mark.parametrize("real,real_output", KINDS)
def test_inverse_is_repeatable(torch, fa, real, real_output):
    """(i) The same inverse ten times into fresh outputs: every result bit-equal to the first."""
    P, T, D, nf, batch = 256, 4, 192, 40, 3
    rt, ct = dtypes(torch, real)
    g = torch.Generator(device="cuda").manual_seed(P)
    Y = spectrum(torch, g, real, (batch, nf, bins_of(P, real_output)))
    h = filter_of(torch, fa, g, real, P, T, prototype=True)
    plan = fa.Ipfb(P, T, real, D, real_output, 0)
    plan.set_filter(h)
    length = plan.length(nf) - 3
    outs = [torch.full((batch, length), float("nan"), dtype=rt if real_output else ct, device="cuda") for _ in range(10)]
    for out in outs:
        plan.inverse(Y, length, out=out)
    torch.cuda.synchronize()
    err = rel_l2(outs[0].cpu().numpy(), truth.synth(Y.cpu().numpy(), h.cpu().numpy(), P, T, D, real_output, length))
    assert err <= tol(plan, real), (real, real_output, err)
    for i, out in enumerate(outs[1:]):
        assert torch.equal(bits(torch, out), bits(torch, outs[0])), (real, real_output, "run", i + 1)


@pytest.mark.parametrize("real_output", [True, False])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, real_output):
    """(j) An inverse captured on a side stream as the first call of a handle that reserved (it must not allocate), one linear graph,
    replayed twice on new input contents: bit-equal to the eager call, and within tolerance of the truth."""
    P, T, D, nf, batch = 256, 4, 192, 10, 3
    g = torch.Generator(device="cuda").manual_seed(12)
    Ys = [spectrum(torch, g, "f32", (batch, nf, bins_of(P, real_output))) for _ in range(3)]
    h = filter_of(torch, fa, g, "f32", P, T)
    side = torch.cuda.Stream()
    other = fa.Ipfb(P, T, "f32", D, real_output, 0)  # loads the kernels' code object (the first launch of a module is not capturable)
    with torch.cuda.stream(side):
        other.inverse(Ys[0])
    side.synchronize()
    plan = fa.Ipfb(P, T, "f32", D, real_output, 0)
    plan.set_filter(h)
    plan.reserve(nf, batch)
    torch.cuda.synchronize()
    d = Ys[0].clone()
    y = torch.empty(batch, plan.length(nf), dtype=torch.float32 if real_output else torch.complex64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.inverse(d, out=y)  # the first call on this plan: captured
    hh = h.cpu().numpy()
    for Y in Ys[1:]:
        d.copy_(Y)
        graph.replay()
        torch.cuda.synchronize()
        ey = plan.inverse(Y)
        torch.cuda.synchronize()
        assert torch.equal(bits(torch, y), bits(torch, ey)), real_output
        assert rel_l2(y.cpu().numpy(), truth.synth(Y.cpu().numpy(), hh, P, T, D, real_output)) <= tol(plan, "f32")


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test (tests/test_gpu_chunks.py): it reads the scratch bound from the
    environment at create.  A handle keeps the library it was created from."""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


@pytest.mark.parametrize("real_output", [True, False])
def test_chunk_walk_under_a_small_scratch_bound(torch, fx, monkeypatch, real_output):
    """(k) P = 250, T = 3, D = 100 (cover 8), 20 frames, batch 3, an odd row length; a frame takes P values of the output's kind in the
    scratch.  Bounds of one frame and of cover() frames: ranges inside every row from cover() frames; a bound of a row's frames plus
    three: whole rows one at a time (tests/test_ipfb_emu.py asserts the cuts).  Bit-equal to a handle of the same library without the
    bound, and within tolerance."""
    P, T, D, nf, batch, real = 250, 3, 100, 20, 3, "f32"
    cover = truth.cover(P, T, D)
    length = truth.full(nf, P, T, D) - 5
    g = torch.Generator(device="cuda").manual_seed(41)
    Y = spectrum(torch, g, real, (batch, nf, bins_of(P, real_output)))
    h = filter_of(torch, fx, g, real, P, T)
    ref = fx.Ipfb(P, T, real, D, real_output, 0)
    ref.set_filter(h)
    y = inverse(torch, ref, Y, length)
    assert rel_l2(y.cpu().numpy(), truth.synth(Y.cpu().numpy(), h.cpu().numpy(), P, T, D, real_output, length)) <= tol(ref, real)
    per = P * (4 if real_output else 8)
    for fit in (1, cover, nf + 3):
        walk = truth.inverse_walk(P, T, D, nf, batch, length, fit)
        assert len(walk) > batch if fit <= cover else len(walk) == batch
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(fit * per))
        try:
            small = fx.Ipfb(P, T, real, D, real_output, 0)
        finally:
            monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_filter(h)
        assert small.describe() == ref.describe()
        got = inverse(torch, small, Y, length)
        assert torch.equal(bits(torch, got), bits(torch, y)), (real_output, fit)


def test_torch_layer(torch, fa):
    """(l)"""
    g = torch.Generator(device="cuda").manual_seed(3)
    P, T, D, nf = 256, 4, 192, 11
    for real in ("f32", "f64"):
        rt, ct = dtypes(torch, real)
        base = 2e-6 if real == "f32" else 1e-13
        for real_output in (True, False):
            bins = bins_of(P, real_output)
            Y = spectrum(torch, g, real, (2, 3, nf, bins))
            h = fa.pfb_prototype(P, T, rt).cuda()
            full = truth.full(nf, P, T, D)
            y = fa.pfb_synthesize(Y, h, P, D, real_output=real_output)
            assert y.shape == (2, 3, full) and y.dtype == (rt if real_output else ct) and y.is_contiguous()
            want = truth.synth(Y.reshape(6, nf, bins).cpu().numpy(), h.cpu().numpy(), P, T, D, real_output).reshape(2, 3, full)
            assert rel_l2(y.cpu().numpy(), want) <= 2 * base
            y2 = fa.pfb_synthesize(Y, h.view(T, P), P, D, real_output=real_output)  # the filter as (taps, channels)
            assert torch.equal(bits(torch, y), bits(torch, y2))
            out = torch.empty(2, 3, full - 9, dtype=y.dtype, device="cuda")
            assert fa.pfb_synthesize(Y, h, P, D, length=full - 9, real_output=real_output, out=out) is out
            assert torch.equal(bits(torch, out), bits(torch, y[..., : full - 9]))
            # defaults: hop = channels, a filter of ones with one tap: the plain inverse DFT of every frame, side by side
            yd = fa.pfb_synthesize(Y[0, 0], None, P, real_output=real_output)
            assert yd.shape == (nf * P,)
            ref = torch.fft.irfft(Y[0, 0], n=P) if real_output else torch.fft.ifft(Y[0, 0])
            assert rel_l2(yd.cpu().numpy(), ref.reshape(-1).cpu().numpy()) <= 4 * base  # two implementations, each within twice the base
    Y = spectrum(torch, g, "f32", (4, nf, P))
    h = torch.ones(P * T, device="cuda")
    with pytest.raises(TypeError):
        fa.pfb_synthesize(Y.cpu(), h, P)
    with pytest.raises(TypeError):
        fa.pfb_synthesize(Y.real.contiguous(), h, P)
    with pytest.raises(TypeError):
        fa.pfb_synthesize(Y, h.double(), P)
    with pytest.raises(ValueError):
        fa.pfb_synthesize(Y, h, P, real_output=True)  # P bins are not the P / 2 + 1 of real rows
    with pytest.raises(ValueError):
        fa.pfb_synthesize(Y[..., : P // 2 + 1], h, P)
    with pytest.raises(ValueError):
        fa.pfb_synthesize(Y, h[:-1], P)
    with pytest.raises(ValueError):
        fa.pfb_synthesize(Y, h, P, hop=0)
    with pytest.raises(ValueError):
        fa.pfb_synthesize(Y, h, P, length=truth.full(nf, P, T, P) + 1)
    with pytest.raises(TypeError):
        fa.Ipfb(P, T, "f32", D, False, 0).inverse(Y, out=torch.empty(4, 7, dtype=torch.complex64, device="cuda"))
