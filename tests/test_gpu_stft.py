"""The STFT handle on the MI355X: fourier_hip_stft_* through the C ABI (Stft.forward_ptr / inverse_ptr) and stft / istft on torch
tensors, against tests/stft_truth.py (f64 numpy on the rounded input).  The CPU twin is tests/test_stft_emu.py (it also covers the
argument checks, the chunk walks and the allocation-free property after reserve).

Tolerance, relative L2 over the whole output: forward twice tests/test_gpu_real.py's tol() for the inner plan's describe string (what
tests/test_gpu_r2r.py grants a transform plus one more rounding stage), inverse and round trip twice that again."""
import numpy as np
import pytest

import stft_truth as truth
from helpers import max_rel, rel_l2

pytestmark = pytest.mark.gpu

FUSED_N = (256, 512, 1024, 2048)
SENTINEL = 77.0


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


def make(fa, real, n_fft, hop, win_length=None, pad_mode="reflect"):
    return fa.Stft(n_fft, real, hop, win_length, pad_mode != "none", "reflect" if pad_mode == "none" else pad_mode, 0)


def has_fused(real, n_fft):
    return n_fft in (128, 256, 512, 1024) or (n_fft == 2048 and real == "f32")


def check_forward(torch, fa, real, n_fft, hop, length, batch, pad_mode="reflect", win_length=None, use_window=True, normalized=False,
                  offset=0):
    """both "fusion" values where the fused route exists, against the truth and each other; describe() says which route ran"""
    plan = make(fa, real, n_fft, hop, win_length, pad_mode)
    g = torch.Generator(device="cuda").manual_seed(n_fft + hop + length)
    w = None
    if use_window:
        w = 0.5 + torch.rand(plan.win_length(), dtype=rdtype(torch, real), device="cuda", generator=g)
    plan.set_window(w)
    base = torch.randn(batch * length + offset, dtype=rdtype(torch, real), device="cuda", generator=g)
    x = base[offset:].view(batch, length)
    assert plan.frames(length) == truth.frames(length, n_fft, hop, pad_mode) > 0
    want = truth.stft(x.cpu().numpy(), n_fft, hop, plan.win_length(), None if w is None else w.cpu().numpy(), pad_mode, normalized)
    got = {}
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        fused = fusion == 1 and has_fused(real, n_fft)
        d = plan.describe()
        assert d.startswith("stft fused rows, istft composed: real half-length: " if fused else "stft composed, istft composed: real "), d
        got[fusion] = plan.forward(x, normalized).cpu().numpy()
        err, emax = rel_l2(got[fusion], want), max_rel(got[fusion], want)
        print(f"stft {real} n_fft={n_fft} hop={hop} length={length} {pad_mode} fusion={fusion}: err {err:.3g} tol {tol(plan, real):.3g} "
              f"max_rel {emax:.3g}")
        assert err <= tol(plan, real), (real, n_fft, hop, length, pad_mode, fusion, err, d)
        # the largest single error over the largest value, within twice the L2 bound (the ratio tests/test_gpu_parity.py grants,
        # tmax = 2 tl2): one wrong element among thousands hides in the L2 norm, not here
        assert emax <= 2 * tol(plan, real), (real, n_fft, hop, length, pad_mode, fusion, emax, d)
    assert rel_l2(got[1], got[0]) <= tol(plan, real)
    return plan


@pytest.mark.parametrize("n_fft", FUSED_N)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_shapes(torch, fa, real, n_fft):
    n = n_fft
    check_forward(torch, fa, real, n, n // 4, 5 * n + 3, 3)                  # frames not a multiple of the tile, a workgroup spans two rows
    check_forward(torch, fa, real, n, 37, 3 * n + 1, 2)                      # frames start on odd elements: single reals
    check_forward(torch, fa, real, n, n + 8, 4 * n, 2)                       # gaps between frames
    check_forward(torch, fa, real, n, n // 4, 4 * n, 2, win_length=n - 56)   # a shorter window, centred
    check_forward(torch, fa, real, n, n // 4, n // 2 + 1, 2)                 # both mirrors in one frame
    for pad_mode in ("none", "constant"):
        check_forward(torch, fa, real, n, n // 2, 3 * n + 10, 2, pad_mode=pad_mode)
    check_forward(torch, fa, real, n, n // 2, 4 * n, 2, normalized=True)
    check_forward(torch, fa, real, n, n // 2, 4 * n, 2, use_window=False)
    check_forward(torch, fa, real, n, n // 4, 4 * n, 2, offset=1)            # the input one element off an allocation


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_composed_only_shapes(torch, fa, real):
    for n, hop, route in ((400, 160, "stockham"), (255, 64, "real full-length"), (382, 100, "bluestein"), (4096, 1024, "stockham")):
        plan = check_forward(torch, fa, real, n, hop, 3 * n + 7, 3)
        assert plan.describe().startswith("stft composed") and route in plan.describe(), plan.describe()


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_inverse_matches_the_truth_and_round_trips(torch, fa, real):
    g = torch.Generator(device="cuda").manual_seed(7)
    dt = rdtype(torch, real)
    for n, hop, pad_mode, nf, cut in ((256, 64, "reflect", 33, 0), (1024, 512, "constant", 9, 17), (400, 160, "none", 12, 3), (255, 50, "reflect", 20, 0)):
        plan = make(fa, real, n, hop, None, pad_mode)
        w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
        plan.set_window(w)
        X = torch.view_as_complex(torch.randn(3, nf, plan.bins(), 2, dtype=dt, device="cuda", generator=g))
        length = plan.default_length(nf) - cut
        for normalized in (False, True):
            got = plan.inverse(X, length, normalized).cpu().numpy()
            want = truth.istft(X.cpu().numpy(), n, hop, length, None, w.cpu().numpy(), pad_mode, normalized)
            err = rel_l2(got, want)
            print(f"istft {real} n_fft={n} hop={hop} {pad_mode}: err {err:.3g} tol {tol(plan, real, True):.3g}")
            assert err <= tol(plan, real, True), (real, n, hop, pad_mode, normalized, err)
    for n in (512, 2048):
        for hop in (n // 4, n // 2):
            for pad_mode in ("reflect", "constant"):
                w = torch.hann_window(n, periodic=True, dtype=dt, device="cuda")
                x = torch.randn(2, 6 * n + 40, dtype=dt, device="cuda", generator=g)
                X = fa.stft(x, n, hop, window=w, pad_mode=pad_mode)
                length = x.shape[-1] - 90  # explicit and shorter than the frames give back
                y = fa.istft(X, n, hop, window=w, length=length)
                err = rel_l2(y.cpu().numpy(), x[:, :length].cpu().numpy())
                base = 2e-6 if real == "f32" else 1e-13
                print(f"round trip {real} n_fft={n} hop={hop} {pad_mode}: err {err:.3g} tol {4 * base:.3g}")
                assert err <= 4 * base, (real, n, hop, pad_mode, err)


def test_nola_refusal(torch, fa):
    n = 256
    plan = make(fa, "f32", n, n, None, "none")  # a Hann window with hop = n_fft: its zero at the frame edge is never covered
    plan.set_window(torch.hann_window(n, periodic=True, dtype=torch.float32, device="cuda"))
    X = torch.zeros(1, 3, plan.bins(), dtype=torch.complex64, device="cuda")
    with pytest.raises(fa.FourierError):
        plan.inverse(X)
    with pytest.raises(fa.FourierError):
        fa.istft(X.transpose(-1, -2), n, n, window=torch.hann_window(n, dtype=torch.float32, device="cuda"), center=False)
    plan.set_window(None)
    assert plan.inverse(X).shape == (1, 3 * n)


def test_torch_layer(torch, fa):
    g = torch.Generator(device="cuda").manual_seed(3)
    for dt, cdt, real in ((torch.float32, torch.complex64, "f32"), (torch.float64, torch.complex128, "f64")):
        n, hop = 512, 128
        x = torch.randn(2, 3, 2000, dtype=dt, device="cuda", generator=g)
        w = torch.hann_window(400, dtype=dt, device="cuda")
        X = fa.stft(x, n, hop, win_length=400, window=w, normalized=True)
        nf = 1 + 2000 // hop
        assert X.shape == (2, 3, n // 2 + 1, nf) and X.dtype == cdt
        # the transposed view of the frame-major buffer: bins contiguous per frame, leading dimensions folded into the batch
        assert X.stride() == (3 * nf * (n // 2 + 1), nf * (n // 2 + 1), 1, n // 2 + 1) and not X.is_contiguous()
        ref = torch.stft(x.reshape(6, 2000), n, hop, 400, w, center=True, pad_mode="reflect", normalized=True, onesided=True,
                         return_complex=True).reshape(2, 3, n // 2 + 1, nf)
        base = 2e-6 if real == "f32" else 1e-13
        assert rel_l2(X.cpu().numpy(), ref.cpu().numpy()) <= 4 * base  # two implementations, each within twice the base of the truth
        y = fa.istft(X, n, hop, win_length=400, window=w, normalized=True, length=1900)
        assert y.shape == (2, 3, 1900) and y.dtype == dt
        assert rel_l2(y.cpu().numpy(), x[..., :1900].cpu().numpy()) <= 4 * base
        y2 = fa.istft(X.contiguous(), n, hop, win_length=400, window=w, normalized=True, length=1900)  # another layout: copied
        assert torch.equal(y, y2)
        # defaults: hop n_fft // 4, a window of ones, the full length
        Xd = fa.stft(x[0, 0], 256)
        assert Xd.shape == (129, 1 + 2000 // 64)
        assert fa.istft(Xd, 256).shape == (64 * (2000 // 64),)
        # out= on the handle
        plan = fa.Stft(n, real, hop, 400, device=0)
        plan.set_window(w)
        out = torch.empty(6, nf, n // 2 + 1, dtype=cdt, device="cuda")
        assert plan.forward(x.reshape(6, 2000), True, out=out) is out
        assert torch.equal(out, X.transpose(-1, -2).reshape(6, nf, n // 2 + 1))
        back = torch.empty(6, 1900, dtype=dt, device="cuda")
        assert plan.inverse(out, 1900, True, out=back) is back and torch.equal(back.view(2, 3, 1900), y)
        with pytest.raises(TypeError):
            plan.forward(x.reshape(6, 2000), out=torch.empty(6, nf, n // 2 + 1, dtype=cdt))
    x = torch.randn(4, 1000, device="cuda")
    with pytest.raises(TypeError):
        fa.stft(x.cpu(), 256)
    with pytest.raises(TypeError):
        fa.stft(x.to(torch.complex64), 256)
    with pytest.raises(TypeError):
        fa.stft(x, 256, window=torch.ones(256, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fa.stft(x, 256, window=torch.ones(255, device="cuda"))
    with pytest.raises(ValueError):
        fa.stft(x, 256, win_length=257)
    with pytest.raises(ValueError):
        fa.stft(x, 256, hop_length=0)
    with pytest.raises(ValueError):
        fa.stft(x, 256, pad_mode="edge")
    with pytest.raises(ValueError):
        fa.stft(x[:, :100], 256)          # reflect needs more than n_fft / 2 samples
    with pytest.raises(ValueError):
        fa.stft(x[:, :100], 256, center=False)
    with pytest.raises(TypeError):
        fa.istft(x, 256)
    with pytest.raises(ValueError):
        fa.istft(torch.zeros(4, 100, 9, dtype=torch.complex64, device="cuda"), 256)
    with pytest.raises(ValueError):
        fa.istft(torch.zeros(4, 129, 9, dtype=torch.complex64, device="cuda"), 256, length=8 * 64 + 1)


@pytest.mark.parametrize("n_fft", [128, 256, 1024])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_input_on_an_odd_element(torch, fa, real, n_fft):
    """The output is complex and always aligned to a pair; the real input is not.  Rows that start one element into their allocation
    (the fused route then loads single reals where it otherwise loads pairs): against the truth, bit-equal to the result from an
    aligned copy of the same rows on the same route, the elements around the output and the input buffer itself untouched."""
    n, hop = n_fft, n_fft // 4
    dt, ct = rdtype(torch, real), torch.complex64 if real == "f32" else torch.complex128
    g = torch.Generator(device="cuda").manual_seed(n)
    length, batch = 3 * n + 2, 2
    base = torch.randn(batch * length + 2, dtype=dt, device="cuda", generator=g)
    before = base.clone()
    x = base[1:-1].view(batch, length)
    xa = x.clone()
    assert x.data_ptr() % (2 * x.element_size()) != 0 and xa.data_ptr() % (2 * x.element_size()) == 0
    plan = make(fa, real, n, hop)
    w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
    plan.set_window(w)
    nf = plan.frames(length)
    want = truth.stft(xa.cpu().numpy(), n, hop, n, w.cpu().numpy(), "reflect")
    count = batch * nf * plan.bins()
    for fusion in (1, 0):
        plan.set_option("fusion", fusion)
        fused = fusion == 1 and has_fused(real, n)
        assert plan.describe().startswith("stft fused rows" if fused else "stft composed"), plan.describe()
        aligned = plan.forward(xa)
        buf = torch.full((count + 2,), SENTINEL, dtype=ct, device="cuda")
        out = buf[1:1 + count].view(batch, nf, plan.bins())
        assert plan.forward(x, out=out) is out
        err, emax = rel_l2(out.cpu().numpy(), want), max_rel(out.cpu().numpy(), want)
        print(f"stft odd input {real} n_fft={n} fusion={fusion}: err {err:.3g} max_rel {emax:.3g} tol {tol(plan, real):.3g}")
        assert err <= tol(plan, real) and emax <= 2 * tol(plan, real), (real, n, fusion, err, emax)
        assert buf[0].item() == SENTINEL and buf[-1].item() == SENTINEL, "an element beside the output was written"
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(aligned)), (real, n, fusion)
        assert torch.equal(base, before), "forward modified its input"


@pytest.mark.parametrize("n_fft", FUSED_N)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fused_forward_is_repeatable(torch, fa, real, n_fft):
    """The same fused forward twenty times into fresh outputs: every result bit-equal to the first (a race on the kernel's LDS
    buffers shows as a difference between runs).  Where the precision has no fused kernel of the length the composed route runs."""
    n, hop = n_fft, n_fft // 4
    g = torch.Generator(device="cuda").manual_seed(n)
    dt, ct = rdtype(torch, real), torch.complex64 if real == "f32" else torch.complex128
    length, batch = 5 * n + 3, 3
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    plan = make(fa, real, n, hop)
    plan.set_option("fusion", 1)
    assert plan.describe().startswith("stft fused rows" if has_fused(real, n) else "stft composed"), plan.describe()
    nf = plan.frames(length)
    outs = [torch.full((batch, nf, plan.bins()), float("nan"), dtype=ct, device="cuda") for _ in range(20)]
    for out in outs:
        plan.forward(x, out=out)
    torch.cuda.synchronize()
    err = rel_l2(outs[0].cpu().numpy(), truth.stft(x.cpu().numpy(), n, hop, n, None, "reflect"))
    assert err <= tol(plan, real), (real, n, err)
    for i, out in enumerate(outs[1:]):
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(outs[0])), (real, n, "run", i + 1)


@pytest.mark.parametrize("fusion", [1, 0])
def test_graph_replay_on_a_side_stream_after_reserve(torch, fa, fusion):
    """Forward and inverse captured on a side stream as the first calls of a handle that reserved (they must not allocate), replayed
    twice on new input contents: bit-equal to the eager calls, and within tolerance of the truth."""
    n, hop, length, batch = 256, 64, 5 * 256, 3  # a length the frames give back in full: reserve() then covers the inverse to it
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randn(batch, length, dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    w = 0.5 + torch.rand(n, dtype=torch.float32, device="cuda", generator=g)
    side = torch.cuda.Stream()
    other = make(fa, "f32", n, hop)  # loads the kernels' code object (the first launch of a module is not capturable)
    other.set_option("fusion", fusion)
    with torch.cuda.stream(side):
        other.inverse(other.forward(xs[0]), length)
    side.synchronize()
    plan = make(fa, "f32", n, hop)
    plan.set_option("fusion", fusion)
    plan.set_window(w)
    assert plan.describe().startswith("stft fused rows" if fusion else "stft composed"), plan.describe()
    plan.reserve(length, batch)
    nf = plan.frames(length)
    torch.cuda.synchronize()
    d = xs[0].clone()
    X = torch.empty(batch, nf, plan.bins(), dtype=torch.complex64, device="cuda")
    y = torch.empty(batch, length, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward(d, out=X)  # the first calls on this plan: captured
        plan.inverse(X, length, out=y)
    wh = w.cpu().numpy()
    for x in xs[1:]:
        d.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eX = plan.forward(x)
        ey = plan.inverse(eX, length)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(X), torch.view_as_real(eX)) and torch.equal(y, ey), fusion
        assert rel_l2(X.cpu().numpy(), truth.stft(x.cpu().numpy(), n, hop, n, wh, "reflect")) <= tol(plan, "f32")
        assert rel_l2(y.cpu().numpy(), truth.istft(X.cpu().numpy(), n, hop, length, None, wh, "reflect")) <= tol(plan, "f32", True)
