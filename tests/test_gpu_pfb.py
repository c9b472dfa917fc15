"""The polyphase filter bank handle on the MI355X: fourier_hip_pfb_* through the C ABI (Pfb.forward_ptr) and pfb_channelize on torch
tensors, against tests/pfb_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_pfb_emu.py (it also covers the argument
checks, the frame count and the allocation-free property after reserve).

Tolerance, relative L2 over the whole output: the STFT tests' forward tolerance, twice tests/test_gpu_real.py's tol() for the inner
plan's describe string (a transform plus one more rounding stage, here the tap sum): 2 x (2e-6 f32, 1e-13 f64; Bluestein inner plans
4e-6 / 1e-11); tests/test_pfb_emu.py shows the tap sum's share of it.  The largest single error stays within twice that."""
import ctypes
import os

import numpy as np
import pytest

import pfb_truth as truth
import stft_truth
from helpers import max_rel, rel_l2

pytestmark = pytest.mark.gpu

COLS = 64  # no tile of the fused kernels holds more frames
SENTINEL = 77.0
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


def has_fused(real, real_input, P):
    h = P // 2 if real_input else P
    return (not real_input or P % 2 == 0) and (h in (64, 128, 256, 512) or (h == 1024 and real == "f32"))


def signal(torch, g, real, real_input, count):
    rt, ct = dtypes(torch, real)
    if real_input:
        return torch.randn(count, dtype=rt, device="cuda", generator=g)
    return torch.view_as_complex(torch.randn(count, 2, dtype=rt, device="cuda", generator=g))


def filter_of(torch, fa, g, real, P, T, prototype=False):
    rt = dtypes(torch, real)[0]
    if prototype:
        return fa.pfb_prototype(P, T, rt).cuda()
    return 0.5 + torch.rand(P * T, dtype=rt, device="cuda", generator=g)


def check(torch, fa, real, real_input, P, T, D, length, batch, use_filter=True, prototype=False, offset=0):
    """both "fusion" values through forward_ptr between guard frames, against the truth and each other; describe() says which route ran"""
    rt, ct = dtypes(torch, real)
    plan = fa.Pfb(P, T, real, D, real_input, 0)
    g = torch.Generator(device="cuda").manual_seed(7 * P + T + D + length)
    h = filter_of(torch, fa, g, real, P, T, prototype) if use_filter else None
    plan.set_filter(h)
    base = signal(torch, g, real, real_input, batch * length + offset)
    before = base.clone()
    x = base[offset:].view(batch, length)
    nf, bins = plan.frames(length), plan.bins()
    assert nf == truth.frames(length, P, T, D) > 0 and bins == (P // 2 + 1 if real_input else P)
    want = truth.pfb(x.cpu().numpy(), None if h is None else h.cpu().numpy(), P, T, D, real_input)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        fused = fusion == 1 and has_fused(real, real_input, P)
        d = plan.describe()
        assert d.startswith("pfb fused rows: " if fused else "pfb composed: "), d
        buf = torch.full((batch * nf + 2, bins), SENTINEL, dtype=ct, device="cuda")
        plan.forward_ptr(x.data_ptr(), buf[1:].data_ptr(), length, batch, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "a guard frame was written"
        assert torch.equal(torch.view_as_real(base) if not real_input else base, torch.view_as_real(before) if not real_input else before), "forward modified its input"
        got[fusion] = buf[1:-1].view(batch, nf, bins).cpu().numpy()
        err, emax = rel_l2(got[fusion], want), max_rel(got[fusion], want)
        print(f"pfb {real} {'real' if real_input else 'complex'} P={P} T={T} D={D} length={length} fusion={fusion}: err {err:.3g} "
              f"tol {tol(plan, real):.3g} max_rel {emax:.3g}  [{d}]")
        assert err <= tol(plan, real), (real, real_input, P, T, D, length, fusion, err, d)
        # the largest single error over the largest value, within twice the L2 bound (tests/test_gpu_stft.py): one wrong element among
        # thousands hides in the L2 norm, not here
        assert emax <= 2 * tol(plan, real), (real, real_input, P, T, D, length, fusion, emax, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("real,real_input", KINDS)
def test_fused_shapes(torch, fa, real, real_input):
    P = 256
    check(torch, fa, real, real_input, P, 4, P, P * 4 + (COLS + 2) * P + 3, 3)                   # (a) frames not a multiple of the tile, a workgroup spans two rows
    check(torch, fa, real, real_input, P, 3, 37, P * 3 + 2 * 37 + 1, 2)                          # (b) odd T; frames on odd elements: single reals
    check(torch, fa, real, real_input, P, 16, 3 * P // 4, P * 16 + 4 * (3 * P // 4), 2, prototype=True)  # (c) oversampled, the longest tap loop
    check(torch, fa, real, real_input, P, 2, P + 8, P * 2 + 2 * (P + 8), 2)                      # (d) gaps between frames
    check(torch, fa, real, real_input, P, 4, P, P * 4 + 3 * P, 2, use_filter=False)              # (f) the default filter of all ones
    check(torch, fa, real, real_input, P, 3, 64, P * 3 + 4 * 64, 2, offset=1)                    # the input one element off an allocation


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_one_tap_is_the_stft_without_padding(torch, fa, real):
    """(e) T = 1, D = P / 2, real rows: the STFT handle with pad_mode none and the filter as its window computes the same thing"""
    P, D = 256, 128
    length = P + 5 * D
    plan = check(torch, fa, real, True, P, 1, D, length, 2)
    g = torch.Generator(device="cuda").manual_seed(8)
    h = filter_of(torch, fa, g, real, P, 1)
    x = signal(torch, g, real, True, 2 * length).view(2, length)
    plan.set_filter(h)
    stft = fa.Stft(P, real, D, None, False, "reflect", 0)
    stft.set_window(h)
    ref = stft.forward(x).cpu().numpy()
    assert rel_l2(ref, stft_truth.stft(x.cpu().numpy(), P, D, P, h.cpu().numpy(), "none")) <= tol(plan, real)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        assert rel_l2(plan.forward(x).cpu().numpy(), ref) <= tol(plan, real), (real, fusion)


@pytest.mark.parametrize("real,real_input", KINDS)
def test_set_filter_null_restores_the_ones(torch, fa, real, real_input):
    """(f)"""
    P, T, D = 256, 2, 256
    g = torch.Generator(device="cuda").manual_seed(9)
    plan = fa.Pfb(P, T, real, D, real_input, 0)
    x = signal(torch, g, real, real_input, P * T + 2 * D).view(1, -1)
    h = filter_of(torch, fa, g, real, P, T)
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        ones = plan.forward(x)
        plan.set_filter(h)
        with_h = plan.forward(x)
        assert rel_l2(with_h.cpu().numpy(), truth.pfb(x.cpu().numpy(), h.cpu().numpy(), P, T, D, real_input)) <= tol(plan, real)
        plan.set_filter(None)
        again = plan.forward(x)
        assert torch.equal(torch.view_as_real(again), torch.view_as_real(ones)) and not torch.equal(torch.view_as_real(with_h), torch.view_as_real(ones))


@pytest.mark.parametrize("real,real_input", KINDS)
def test_the_other_fused_sizes(torch, fa, real, real_input):
    """(g) one case per other fused P of the kind; f64 at the top size stays composed (has_fused, asserted through describe())"""
    k = 2 if real_input else 1
    for P in (64 * k, 128 * k, 512 * k):
        check(torch, fa, real, real_input, P, 2, P, P * 2 + COLS * P, 1)
    assert has_fused(real, real_input, 1024 * k) == (real == "f32")
    check(torch, fa, real, real_input, 1024 * k, 2, 1024 * k, 1024 * k * 2 + 8 * 1024 * k, 1)


@pytest.mark.parametrize("real,real_input", KINDS)
def test_composed_only_shapes(torch, fa, real, real_input):
    for P in (400, 4096):
        plan = check(torch, fa, real, real_input, P, 3, 3 * P // 4, 3 * P + 2 * (3 * P // 4) + 5, 2)
        assert plan.describe().startswith("pfb composed") and "stockham" in plan.describe(), plan.describe()


@pytest.mark.parametrize("real,real_input", KINDS)
def test_forward_is_repeatable(torch, fa, real, real_input):
    """The same fused forward ten times into fresh outputs: every result bit-equal to the first (a race on the kernel's LDS buffers
    shows as a difference between runs)."""
    P, T, D = 256, 4, 192
    ct = dtypes(torch, real)[1]
    g = torch.Generator(device="cuda").manual_seed(P)
    length, batch = P * T + 40 * D + 3, 3
    x = signal(torch, g, real, real_input, batch * length).view(batch, length)
    h = filter_of(torch, fa, g, real, P, T, prototype=True)
    plan = fa.Pfb(P, T, real, D, real_input, 0)
    plan.set_filter(h)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("pfb fused rows"), plan.describe()
    outs = [torch.full((batch, plan.frames(length), plan.bins()), float("nan"), dtype=ct, device="cuda") for _ in range(10)]
    for out in outs:
        plan.forward(x, out=out)
    torch.cuda.synchronize()
    err = rel_l2(outs[0].cpu().numpy(), truth.pfb(x.cpu().numpy(), h.cpu().numpy(), P, T, D, real_input))
    assert err <= tol(plan, real), (real, real_input, err)
    for i, out in enumerate(outs[1:]):
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(outs[0])), (real, real_input, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """A forward captured on a side stream as the first call of a handle that reserved (it must not allocate), one linear graph,
    replayed twice on new input contents: bit-equal to the eager call, and within tolerance of the truth."""
    P, T, D, batch = 256, 4, 192, 3
    length = P * T + 9 * D
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randn(batch, length, dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    h = filter_of(torch, fa, g, "f32", P, T)
    side = torch.cuda.Stream()
    other = fa.Pfb(P, T, "f32", D, True, 0)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.forward(xs[0])
    side.synchronize()
    plan = fa.Pfb(P, T, "f32", D, True, 0)
    plan.set_option("fusion", fusion)
    plan.set_filter(h)
    assert plan.describe().startswith("pfb fused rows" if fusion else "pfb composed"), plan.describe()
    plan.reserve(length, batch)
    torch.cuda.synchronize()
    d = xs[0].clone()
    X = torch.empty(batch, plan.frames(length), plan.bins(), dtype=torch.complex64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(d, out=X)  # the first call on this plan: captured
    hh = h.cpu().numpy()
    for x in xs[1:]:
        d.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eX = plan.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(X), torch.view_as_real(eX)), fusion
        assert rel_l2(X.cpu().numpy(), truth.pfb(x.cpu().numpy(), hh, P, T, D, True)) <= tol(plan, "f32")


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    P, T, D = 256, 4, 192
    for real in ("f32", "f64"):
        rt, ct = dtypes(torch, real)
        for real_input in (True, False):
            x = signal(torch, g, real, real_input, 2 * 3 * 3000).view(2, 3, 3000)
            h = fa.pfb_prototype(P, T, rt).cuda()
            nf = truth.frames(3000, P, T, D)
            bins = P // 2 + 1 if real_input else P
            X = fa.pfb_channelize(x, h, P, D)
            assert X.shape == (2, 3, nf, bins) and X.dtype == ct and X.is_contiguous()
            want = truth.pfb(x.reshape(6, 3000).cpu().numpy(), h.cpu().numpy(), P, T, D, real_input).reshape(2, 3, nf, bins)
            base = 2e-6 if real == "f32" else 1e-13
            assert rel_l2(X.cpu().numpy(), want) <= 2 * base
            X2 = fa.pfb_channelize(x, h.view(T, P), P, D)  # the filter as (taps, channels)
            assert torch.equal(torch.view_as_real(X), torch.view_as_real(X2))
            out = torch.empty(2, 3, nf, bins, dtype=ct, device="cuda")
            assert fa.pfb_channelize(x, h, P, D, out=out) is out and torch.equal(torch.view_as_real(out), torch.view_as_real(X))
            # defaults: hop = channels, a filter of ones with one tap: the plain DFT of consecutive blocks
            Xd = fa.pfb_channelize(x[0, 0], None, P)
            assert Xd.shape == (3000 // P, bins)
            blocks = x[0, 0, : (3000 // P) * P].view(-1, P)
            ref = torch.fft.rfft(blocks) if real_input else torch.fft.fft(blocks)
            assert rel_l2(Xd.cpu().numpy(), ref.cpu().numpy()) <= 4 * base  # two implementations, each within twice the base of the truth
    x = torch.randn(4, 3000, device="cuda")
    h = torch.ones(P * T, device="cuda")
    with pytest.raises(TypeError):
        fa.pfb_channelize(x.cpu(), h, P)
    with pytest.raises(TypeError):
        fa.pfb_channelize(x.to(torch.int32), h, P)
    with pytest.raises(TypeError):
        fa.pfb_channelize(x, h.double(), P)
    with pytest.raises(ValueError):
        fa.pfb_channelize(x, h[:-1], P)
    with pytest.raises(ValueError):
        fa.pfb_channelize(x, h, P, hop=0)
    with pytest.raises(ValueError):
        fa.pfb_channelize(x[:, : P * T - 1], h, P)
    with pytest.raises(TypeError):
        fa.Pfb(P, T, "f32", D, True, 0).forward(x, out=torch.empty(4, 1, P // 2 + 1, dtype=torch.complex64))


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


@pytest.mark.parametrize("real_input", [True, False])
def test_chunk_walk_under_a_small_scratch_bound(torch, fx, monkeypatch, real_input):
    """Scratch bytes per frame: P values of the input's kind.  Bounds of one and of seven frames: chunks of the flat frame index whose
    boundaries fall inside a row (a.first != 0).  Bit-equal to a handle of the same library without the bound, and within tolerance."""
    P, T, D, batch, real = 250, 3, 100, 3, "f32"
    length = P * T + 10 * D + 5
    g = torch.Generator(device="cuda").manual_seed(41)
    x = signal(torch, g, real, real_input, batch * length).view(batch, length)
    h = filter_of(torch, fx, g, real, P, T)
    ref = fx.Pfb(P, T, real, D, real_input, 0)
    ref.set_filter(h)
    assert ref.describe().startswith("pfb composed"), ref.describe()
    X = ref.forward(x)
    want = truth.pfb(x.cpu().numpy(), h.cpu().numpy(), P, T, D, real_input)
    assert rel_l2(X.cpu().numpy(), want) <= tol(ref, real)
    per = P * (4 if real_input else 8)
    nf = ref.frames(length)
    for frames_in_scratch in (1, 7):
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(frames_in_scratch * per))
        try:
            small = fx.Pfb(P, T, real, D, real_input, 0)
        finally:
            monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        small.set_filter(h)
        assert small.describe() == ref.describe() and batch * nf > frames_in_scratch
        buf = torch.full((batch * nf + 2, small.bins()), SENTINEL, dtype=X.dtype, device="cuda")
        out = buf[1:-1].view(batch, nf, small.bins())
        small.forward(x, out=out)
        torch.cuda.synchronize()
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "a guard frame was written"
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(X)), (real_input, frames_in_scratch)
