"""The handles' chunk walks on the MI355X.  Every handle family that runs through a bounded scratch (RealPlan, R2RPlan, StftPlan,
MdctPlan, SpectrogramPlan, CsdPlan, ConvPlan, LinearConvPlan, RealNdPlan, the transpose route of the axis plan) cuts a call that does not
fit the bound into chunks; the product library's bound is 1 GiB, so at test shapes it runs one chunk.  fourier_amd/lib/libfourier_experiments.so is built
from the same objects and reads the bound from the environment at create (scratch_bound, handle_common.h), which brings the walks --
other grids of every launch, a second scratch half on an 8-byte and not 16-byte aligned address, seam frames transformed twice -- down
to shapes of a few thousand elements.  The CPU twins are the chunk tests of tests/test_*_emu.py.

Every case compares a handle created under a small bound against
  (a) the family's f64 truth, within the tolerance the family's own GPU test grants (restated here from tol() of test_gpu_real.py,
      test_gpu_r2r.py, test_gpu_stft.py, test_gpu_mdct.py, test_gpu_conv.py, test_gpu_lconv.py, test_gpu_realnd.py, test_gpu_axis.py;
      tests/chunk_walks.py restates those of test_gpu_spectrogram.py and test_gpu_csd.py), and
  (b) the result of a handle of the same library created without the bound, on the same input buffers, bit for bit.  The Welch
      average, the cross spectrum and the coherence sum over frames: where a chunk ends inside a slot of partials the sum is
      re-associated, and (b) becomes the bound tests/chunk_walks.py derives for that.
How many chunks a case walks follows from the bound and the per-row scratch bytes stated beside it (the formulas of the plans'
prepare()); each case asserts that the call is larger than one chunk.  Outputs lie between guard elements that must stay untouched."""
import ctypes
import os

import numpy as np
import pytest

import chunk_walks
import mdct_truth
import r2r_truth
import stft_truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

REAL = "FOURIER_REAL_SCRATCH_BYTES"
CONV = "FOURIER_CONV_SCRATCH_BYTES"
REALND = "FOURIER_REALND_SCRATCH_BYTES"
AXIS = "FOURIER_AXIS_SCRATCH_BYTES"
GUARD = 64       # guard elements on either side of an output: keeps the output's alignment that of an allocation
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


@pytest.fixture
def fx(torch, fa):
    """fourier_amd bound to the experiments library for one test; a handle keeps the library it was created from, so the handles
    are created directly and never through the cached tensor entry points."""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


def bounded(monkeypatch, create, **env):
    """create() with the development switches `env` set: they are read at create only"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return create()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def base_tol(describe, real):
    """tests/test_gpu_real.py's tol(): one transform of the inner plan"""
    blu = "bluestein" in describe
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def rdt(torch, real):
    return torch.float32 if real == "f32" else torch.float64


def cdt(torch, real):
    return torch.complex64 if real == "f32" else torch.complex128


def elem(real):
    """bytes of one complex value"""
    return 8 if real == "f32" else 16


class Guarded:
    """an output of `shape` between GUARD sentinel elements in one allocation"""

    def __init__(self, torch, shape, dtype):
        count = int(np.prod(shape))
        self.buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.out = self.buf[GUARD:GUARD + count].view(*shape)
        self.out.fill_(float("nan"))

    def checked(self):
        lo, hi = self.buf[:GUARD].cpu().numpy(), self.buf[-GUARD:].cpu().numpy()
        assert np.all(lo == SENTINEL) and np.all(hi == SENTINEL), "a guard element was written"
        return self.out


def randn(torch, g, shape, dtype):
    if dtype.is_complex:
        return torch.view_as_complex(torch.randn(*shape, 2, dtype=torch.float32 if dtype == torch.complex64 else torch.float64,
                                                 device="cuda", generator=g))
    return torch.randn(*shape, dtype=dtype, device="cuda", generator=g)


# ---- MDCT
@pytest.mark.parametrize("n", [64, 9, 250])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_mdct(torch, fx, monkeypatch, real, n):
    """Scratch bytes per frame: even n two halves of h complex values (n * ELEM), odd n 2n complex values.  n = 250: h = 125, so with an
    odd number of frames per chunk the second half starts 8 bytes off a 16-byte boundary in f32.  Forward chunks are ranges of the flat
    frame index (1, 2, 3 frames: boundaries inside a row, a.first != 0; one row's frames: three chunks); the inverse walks ranges of
    output samples over at least two frames (seam frames transformed twice), or whole rows, one per chunk."""
    dt = rdt(torch, real)
    g = torch.Generator(device="cuda").manual_seed(21 + n)
    length, batch = 9 * n + 5, 3
    per = (n if n % 2 == 0 else 2 * n) * elem(real)
    w = 0.5 + torch.rand(2 * n, dtype=dt, device="cuda", generator=g)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    for center in (True, False):
        ref = fx.Mdct(n, real, center, 0)
        ref.set_option("fusion", 0)
        ref.set_window(w)
        nf = ref.frames(length)
        assert nf == mdct_truth.frames(length, n, center) == (11 if center else 8)
        X = ref.forward(x)
        tf, ti = 2 * base_tol(ref.describe(), real), 4 * base_tol(ref.describe(), real)
        err = rel_l2(X.cpu().numpy(), mdct_truth.mdct(x.cpu().numpy(), n, w.cpu().numpy(), center))
        print(f"mdct chunks {real} n={n} center={center}: unchunked forward err {err:.3g} tol {tf:.3g}  [{ref.describe()}]")
        assert err <= tf, (real, n, center, err)
        backs = [min(length, ref.default_length(nf))]
        backs.append(backs[0] - 5)
        y, want_y = {}, {}
        for back in backs:
            y[back] = ref.inverse(X, back)
            want_y[back] = mdct_truth.imdct(X.cpu().numpy(), n, back, w.cpu().numpy(), center)
            err = rel_l2(y[back].cpu().numpy(), want_y[back])
            print(f"mdct chunks {real} n={n} center={center} back={back}: unchunked inverse err {err:.3g} tol {ti:.3g}")
            assert err <= ti, (real, n, center, back, err)
        for frames_in_scratch in (1, 2, 3, nf):
            small = bounded(monkeypatch, lambda: fx.Mdct(n, real, center, 0), **{REAL: frames_in_scratch * per})
            small.set_option("fusion", 0)
            small.set_window(w)
            assert small.describe() == ref.describe()
            # forward: batch * nf frames in chunks of frames_in_scratch; inverse: ranges over max(2, frames_in_scratch) < nf frames, or
            # (frames_in_scratch == nf) one whole row per chunk of a batch of three
            assert batch * nf > frames_in_scratch and (nf > max(2, frames_in_scratch) or (frames_in_scratch == nf and batch > 1))
            out = Guarded(torch, (batch, nf, n), dt)
            small.forward(x, out=out.out)
            got = out.checked()
            err = rel_l2(got.cpu().numpy(), mdct_truth.mdct(x.cpu().numpy(), n, w.cpu().numpy(), center))
            assert err <= tf, (real, n, center, frames_in_scratch, err)
            assert torch.equal(got, X), ("forward", real, n, center, frames_in_scratch)
            for back in backs:
                out = Guarded(torch, (batch, back), dt)
                small.inverse(X, back, out=out.out)
                got = out.checked()
                err = rel_l2(got.cpu().numpy(), want_y[back])
                assert err <= ti, (real, n, center, frames_in_scratch, back, err)
                assert torch.equal(got, y[back]), ("inverse", real, n, center, frames_in_scratch, back)


def test_mdct_scratch_that_grows_between_calls(torch, fa):
    """The product library: a handle whose scratch grows between a call of one row and a call of three gives what a handle that
    reserved first gives, bit for bit (a pointer into the scratch taken before it grew would show here)."""
    from fourier_amd import _lib

    n, length = 250, 9 * 250 + 5
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(3, length, dtype=torch.float32, device="cuda", generator=g)
    grown = fa.Mdct(n, "f32", True, 0)
    assert grown._L is _lib.lib() and grown._L._name.endswith("libfourier.so")
    one = grown.forward(x[:1])
    three = grown.forward(x)
    back1 = grown.inverse(one, length)
    back3 = grown.inverse(three, length)
    fresh = fa.Mdct(n, "f32", True, 0)
    fresh.reserve(length, 3)
    want = fresh.forward(x)
    assert torch.equal(three, want) and torch.equal(one, want[:1])
    want_back = fresh.inverse(want, length)
    assert torch.equal(back3, want_back) and torch.equal(back1, want_back[:1])
    err = rel_l2(three.cpu().numpy(), mdct_truth.mdct(x.cpu().numpy(), n, mdct_truth.sine_window(n, np.float32)))
    assert err <= 2 * base_tol(fresh.describe(), "f32"), err
    err = rel_l2(back3.cpu().numpy(), x.cpu().numpy())  # the sine window reconstructs
    assert err <= 4 * base_tol(fresh.describe(), "f32"), err


# ---- STFT
@pytest.mark.parametrize("n_fft", [64, 250, 63])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_stft(torch, fx, monkeypatch, real, n_fft):
    """Scratch bytes per frame: n_fft reals.  A bound of one frame: one frame per forward chunk.  The inverse never holds fewer than
    k = ceil(n_fft / hop) frames (its floor: every frame that covers a sample); bounds of k and k + 3 frames walk ranges of output
    samples with the seam frames transformed twice.  The inner RealPlan reads the same bound: at n_fft = 63 (odd: n_fft complex values
    per row) it holds half as many rows as the STFT's scratch and walks chunks of its own inside every STFT chunk."""
    n = n_fft
    dt = rdt(torch, real)
    g = torch.Generator(device="cuda").manual_seed(31 + n)
    length, batch = 9 * n + 5, 3
    per = n * (4 if real == "f32" else 8)
    w = 0.5 + torch.rand(n, dtype=dt, device="cuda", generator=g)
    x = torch.randn(batch, length, dtype=dt, device="cuda", generator=g)
    for hop in (n // 4, n // 3 + 1):
        k = -(-n // hop)
        for pad_mode in ("reflect", "none"):
            make = lambda: fx.Stft(n, real, hop, None, pad_mode != "none", "reflect", 0)  # noqa: E731
            ref = make()
            ref.set_option("fusion", 0)
            ref.set_window(w)
            assert ref.describe().startswith("stft composed, istft composed: real "), ref.describe()
            nf = ref.frames(length)
            assert nf == stft_truth.frames(length, n, hop, pad_mode) > k + 3
            tf, ti = 2 * base_tol(ref.describe(), real), 4 * base_tol(ref.describe(), real)
            X = ref.forward(x)
            want_X = stft_truth.stft(x.cpu().numpy(), n, hop, n, w.cpu().numpy(), pad_mode)
            err = rel_l2(X.cpu().numpy(), want_X)
            print(f"stft chunks {real} n_fft={n} hop={hop} {pad_mode}: unchunked forward err {err:.3g} tol {tf:.3g}  [{ref.describe()}]")
            assert err <= tf, (real, n, hop, pad_mode, err)
            back = ref.default_length(nf)
            y = ref.inverse(X, back)
            want_y = stft_truth.istft(X.cpu().numpy(), n, hop, back, None, w.cpu().numpy(), pad_mode)
            err = rel_l2(y.cpu().numpy(), want_y)
            print(f"stft chunks {real} n_fft={n} hop={hop} {pad_mode}: unchunked inverse err {err:.3g} tol {ti:.3g}")
            assert err <= ti, (real, n, hop, pad_mode, err)
            for frames_in_scratch in (1, k, k + 3):
                small = bounded(monkeypatch, make, **{REAL: frames_in_scratch * per})
                small.set_option("fusion", 0)
                small.set_window(w)
                assert small.describe() == ref.describe()
                assert nf > max(k, frames_in_scratch)  # forward: chunks of frames_in_scratch frames; inverse: ranges of one row
                out = Guarded(torch, (batch, nf, small.bins()), cdt(torch, real))
                small.forward(x, out=out.out)
                got = out.checked()
                err = rel_l2(got.cpu().numpy(), want_X)
                assert err <= tf, (real, n, hop, pad_mode, frames_in_scratch, err)
                assert torch.equal(torch.view_as_real(got), torch.view_as_real(X)), ("forward", real, n, hop, pad_mode, frames_in_scratch)
                out = Guarded(torch, (batch, back), dt)
                small.inverse(X, back, out=out.out)
                got = out.checked()
                err = rel_l2(got.cpu().numpy(), want_y)
                assert err <= ti, (real, n, hop, pad_mode, frames_in_scratch, err)
                assert torch.equal(got, y), ("inverse", real, n, hop, pad_mode, frames_in_scratch)


# ---- power spectrogram, Welch average, cross-spectral density and coherence
class DeviceApi:
    """tests/chunk_walks.py's adapter for the experiments library: handles created under bounded(), inputs on the device, every
    output inside Guarded, results back as numpy arrays"""

    def __init__(self, torch, fx, monkeypatch):
        self.torch, self.fx, self.monkeypatch = torch, fx, monkeypatch

    def _create(self, cls, real, n_fft, hop, pad_mode, w, bound, fusion):
        create = lambda: cls(n_fft, real, hop, None, pad_mode != "none", "reflect", 0)  # noqa: E731
        plan = create() if bound is None else bounded(self.monkeypatch, create, **{REAL: bound})
        plan.set_option("fusion", fusion)
        plan.set_window(self.put(w))
        return plan

    def spectrogram(self, real, n_fft, hop, pad_mode, w, bound, fusion=0):
        return self._create(self.fx.Spectrogram, real, n_fft, hop, pad_mode, w, bound, fusion)

    def cross_spectrum(self, real, n_fft, hop, pad_mode, w, bound, fusion=0):
        return self._create(self.fx.CrossSpectrum, real, n_fft, hop, pad_mode, w, bound, fusion)

    def put(self, a):
        return self.torch.from_numpy(a).cuda()

    def _run(self, call, shape, dtype):
        out = Guarded(self.torch, shape, dtype)
        call(out.out)
        return out.checked().cpu().numpy()

    def forward(self, plan, x, batch, length, power, normalized):
        return self._run(lambda out: plan.forward(x, power, normalized, out=out), (batch, plan.frames(length), plan.bins()), x.dtype)

    def welch(self, plan, x, batch, length, fold, scale):
        return self._run(lambda out: plan.welch(x, fold, scale, out=out), (batch, plan.bins()), x.dtype)

    def csd(self, plan, x, y, batch, length, fold, scale):
        return self._run(lambda out: plan.csd(x, y, fold, scale, out=out), (batch, plan.bins()),
                         self.torch.complex64 if x.dtype == self.torch.float32 else self.torch.complex128)

    def coherence(self, plan, x, y, batch, length):
        return self._run(lambda out: plan.coherence(x, y, out=out), (batch, plan.bins()), x.dtype)


@pytest.mark.parametrize("n_fft", chunk_walks.N_FFTS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_spectrogram_and_welch(torch, fx, monkeypatch, real, n_fft):
    """Scratch bytes per frame: bins * ELEM + n_fft * sizeof(T), the transformed frames first and the windowed frames behind
    chunk * bins complex values; one row of partials: tiles * bins * sizeof(T).  64 frames a row under bounds of 32, 64 and 96 frames
    (chunks end on slot boundaries, 96 inside a row: forward and Welch bit-equal to the unbounded handle); 35 frames a row under bounds
    of 1, 2, 3, 7, 20, 35 and 40 frames (chunks end inside slots: a later launch adds to what an earlier one wrote).  The cases, the
    walk each bound gives and the assertions are chunk_walks.spectrogram_chunks, which the CPU emulation runs too."""
    chunk_walks.spectrogram_chunks(DeviceApi(torch, fx, monkeypatch), real, n_fft)


@pytest.mark.parametrize("n_fft", chunk_walks.N_FFTS)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_csd_and_coherence(torch, fx, monkeypatch, real, n_fft):
    """Scratch bytes per frame pair: 2 * (bins * ELEM + n_fft * sizeof(T)), the y frames behind the chunk's ng x frames on both sides of
    the transform (ystride = ng * bins); one row of partials: tiles * CSD_PLANES * bins * sizeof(T).  The shapes and bounds of
    test_spectrogram_and_welch, in frame pairs; the smallest bounds also cut the batch into row groups.  The cases, the walk each
    bound gives and the assertions are chunk_walks.csd_chunks, which the CPU emulation runs too."""
    chunk_walks.csd_chunks(DeviceApi(torch, fx, monkeypatch), real, n_fft)


@pytest.mark.parametrize("n_fft,fused", [(64, False), (250, False), (63, False), (256, True)])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_welch_row_groups(torch, fx, monkeypatch, real, n_fft, fused):
    """A batch of five under a bound of 8 bytes (rows one by one, one frame per chunk) and of exactly two rows of partials (groups of
    2, 2 and 1 rows), every group through the same partials buffer, an odd and an even row length; n_fft = 256 on the fused route,
    bit-equal to the unbounded fused handle (chunk_walks.welch_groups)."""
    chunk_walks.welch_groups(DeviceApi(torch, fx, monkeypatch), real, n_fft, fused)


@pytest.mark.parametrize("n_fft,fused", [(64, False), (250, False), (63, False), (256, True)])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_csd_row_groups(torch, fx, monkeypatch, real, n_fft, fused):
    """test_welch_row_groups for the cross spectrum and the coherence: the fused route takes its bases from x and from y again for
    every group (chunk_walks.csd_groups)."""
    chunk_walks.csd_groups(DeviceApi(torch, fx, monkeypatch), real, n_fft, fused)


# ---- real-input transforms and DCT / DST
@pytest.mark.parametrize("n", [250, 1001, 4096])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_rfft(torch, fx, monkeypatch, real, n):
    """Scratch bytes per row: even n h complex values, odd n (the full-length inner plan) n.  Two rows per chunk: a batch of seven in
    four chunks, the last one a single row."""
    batch, rows = 7, 2
    per = (n // 2 if n % 2 == 0 else n) * elem(real)
    g = torch.Generator(device="cuda").manual_seed(41 + n)
    x = torch.randn(batch, n, dtype=rdt(torch, real), device="cuda", generator=g)
    S = randn(torch, g, (batch, n // 2 + 1), cdt(torch, real))
    S[:, 0] = S[:, 0].real  # a half spectrum of a real row: bin 0 and, even n, bin n / 2 are real
    if n % 2 == 0:
        S[:, -1] = S[:, -1].real
    ref = fx.RealFft(n, real, 0)
    small = bounded(monkeypatch, lambda: fx.RealFft(n, real, 0), **{REAL: rows * per})
    assert small.describe() == ref.describe() and batch > rows
    t = base_tol(ref.describe(), real)
    stream = torch.cuda.current_stream().cuda_stream
    X = torch.empty(batch, n // 2 + 1, dtype=cdt(torch, real), device="cuda")
    ref.forward_batch_ptr(x.data_ptr(), X.data_ptr(), batch, stream=stream)
    out = Guarded(torch, (batch, n // 2 + 1), cdt(torch, real))
    small.forward_batch_ptr(x.data_ptr(), out.out.data_ptr(), batch, stream=stream)
    got = out.checked()
    want = np.fft.rfft(x.cpu().numpy().astype(np.float64), axis=-1)
    err = rel_l2(got.cpu().numpy(), want)
    print(f"rfft chunks {real} n={n}: forward err {err:.3g} tol {t:.3g}  [{ref.describe()}]")
    assert err <= t and rel_l2(X.cpu().numpy(), want) <= t, (real, n, err)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(X)), ("forward", real, n)
    y = torch.empty(batch, n, dtype=rdt(torch, real), device="cuda")
    ref.inverse_batch_ptr(S.data_ptr(), y.data_ptr(), batch, stream=stream)
    out = Guarded(torch, (batch, n), rdt(torch, real))
    small.inverse_batch_ptr(S.data_ptr(), out.out.data_ptr(), batch, stream=stream)
    got = out.checked()
    want = np.fft.irfft(S.cpu().numpy().astype(np.complex128), n=n, axis=-1)
    err = rel_l2(got.cpu().numpy(), want)
    print(f"rfft chunks {real} n={n}: inverse err {err:.3g} tol {t:.3g}")
    assert err <= t and rel_l2(y.cpu().numpy(), want) <= t, (real, n, err)
    assert torch.equal(got, y), ("inverse", real, n)


@pytest.mark.parametrize("n", [250, 1001, 4096])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_r2r(torch, fx, monkeypatch, real, n):
    """Scratch bytes per row: even n both halves of h complex values, odd n n complex values.  Two rows per chunk: a batch of seven in
    four chunks, the last one a single row; every kind, out of place and in place (a chunk is read completely before it is written)."""
    batch, rows = 7, 2
    per = (2 * (n // 2) if n % 2 == 0 else n) * elem(real)
    g = torch.Generator(device="cuda").manual_seed(51 + n)
    dt = rdt(torch, real)
    x = torch.randn(batch, n, dtype=dt, device="cuda", generator=g)
    xh = x.cpu().numpy()
    ref = fx.R2R(n, real, 0)
    small = bounded(monkeypatch, lambda: fx.R2R(n, real, 0), **{REAL: rows * per})
    assert small.describe() == ref.describe() and batch > rows
    t = 2 * base_tol(ref.describe(), real)
    for kind in r2r_truth.KINDS:
        for norm in ("backward", "ortho"):
            y = ref.transform(x, r2r_truth.KINDS[kind], r2r_truth.NORMS[norm])
            out = Guarded(torch, (batch, n), dt)
            small.transform(x, r2r_truth.KINDS[kind], r2r_truth.NORMS[norm], out=out.out)
            got = out.checked()
            idx, want = r2r_truth.want(kind, norm, xh)
            err = rel_l2(got.cpu().numpy()[:, idx], want)
            print(f"r2r chunks {real} n={n} {kind} {norm}: err {err:.3g} tol {t:.3g}  [{ref.describe()}]")
            assert err <= t and rel_l2(y.cpu().numpy()[:, idx], want) <= t, (real, n, kind, norm, err)
            assert torch.equal(got, y), (real, n, kind, norm)
            z = x.clone()
            small.transform(z, r2r_truth.KINDS[kind], r2r_truth.NORMS[norm], out=z)
            assert torch.equal(z, y), ("in place", real, n, kind, norm)
    assert np.array_equal(x.cpu().numpy(), xh)


# ---- circular and linear convolution
def conv_dtype(torch, real, real_data):
    return rdt(torch, real) if real_data else cdt(torch, real)


def conv_want(x, h):
    """numpy in f64; row b with filter b mod F (tests/test_gpu_conv.py's want)"""
    n = x.shape[-1]
    hb = h[np.arange(x.shape[0]) % h.shape[0]]
    if np.iscomplexobj(x):
        return np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * np.fft.fft(hb.astype(np.complex128), n, axis=-1), axis=-1)
    return np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=-1) * np.fft.rfft(hb.astype(np.float64), n, axis=-1), n=n, axis=-1)


def same_bits(torch, a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fftconv(torch, fx, monkeypatch, real, real_data):
    """Scratch bytes per row: real data n / 2 + 1 complex values on both routes, complex data n on the composed route.  Two filters, a
    batch of five, one and two rows per chunk: five and three chunks of apply, and the filter of a row counts over the whole call.
    The bank is built through the same scratch, a chunk of filters at a time.  Complex n = 4096 is the one-launch route, which has no
    scratch and takes the batch in one launch whatever the bound: it must be unchanged by the bound, and its composed twin
    ("fusion" = 0) walks."""
    dt = conv_dtype(torch, real, real_data)
    batch, F, taps = 5, 2, 33
    for n in (4096, 1000):
        g = torch.Generator(device="cuda").manual_seed(61 + n)
        x = randn(torch, g, (batch, n), dt)
        h = randn(torch, g, (F, taps), dt)
        want = conv_want(x.cpu().numpy(), h.cpu().numpy())
        per = (n // 2 + 1 if real_data else n) * elem(real)
        first = "conv real fused untangle: " if real_data else "conv one-launch: " if n == 4096 else "conv composed: "
        ref = fx.FftConv(n, real, real_data, 0)
        for rows in (1, 2):
            small = bounded(monkeypatch, lambda: fx.FftConv(n, real, real_data, 0), **{CONV: rows * per})
            assert batch > rows
            for fusion in (1, 0):
                for plan in (ref, small):
                    plan.set_option("fusion", fusion)
                    plan.set_filters(h)
                d = small.describe()
                assert d == ref.describe() and d.startswith(first if fusion else "conv real composed: " if real_data else "conv composed: "), d
                t = 3 * base_tol(d, real)
                y = ref.apply(x)
                out = Guarded(torch, (batch, n), dt)
                small.apply(x, out=out.out)
                got = out.checked()
                err = rel_l2(got.cpu().numpy(), want)
                print(f"conv chunks {real} {'real' if real_data else 'complex'} n={n} rows={rows} fusion={fusion}: err {err:.3g} tol {t:.3g}  [{d}]")
                assert err <= t and rel_l2(y.cpu().numpy(), want) <= t, (real, real_data, n, rows, fusion, err)
                assert same_bits(torch, got, y), (real, real_data, n, rows, fusion)
                z = x.clone()
                small.apply(z, out=z)
                assert same_bits(torch, z, y), ("in place", real, real_data, n, rows, fusion)


def lconv_want(x, h, mode):
    """numpy.convolve in f64, row b with filter b mod F, sliced as include/fourier.h says (tests/test_gpu_lconv.py's want)"""
    lx, k = x.shape[-1], h.shape[-1]
    wide = np.complex128 if np.iscomplexobj(x) else np.float64
    off, lout = {"full": (0, lx + k - 1), "valid": (k - 1, lx - k + 1)}[mode]
    return np.array([np.convolve(x[b].astype(wide), h[b % h.shape[0]].astype(wide))[off:off + lout] for b in range(x.shape[0])])


@pytest.mark.parametrize("real_data", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_lconv(torch, fx, monkeypatch, real, real_data):
    """Lx = 5000, K = 129: overlap-save on blocks of 2048.  That route's apply has no scratch; its bank is built through the scratch, a
    chunk of filters of 2048 complex values each at a time, so a bound of one row walks the two filters in two chunks (a bound of two
    rows holds both: the same arithmetic in one chunk).  The padded route ("overlap_save" = 0, M = 8192) walks the batch of five through
    the scratch in rows of M values, one and two rows per chunk."""
    dt = conv_dtype(torch, real, real_data)
    lx, k, batch, F = 5000, 129, 5, 2
    g = torch.Generator(device="cuda").manual_seed(71)
    x = randn(torch, g, (batch, lx), dt)
    h = randn(torch, g, (F, k), dt)
    xh, hh = x.cpu().numpy(), h.cpu().numpy()
    for mode in ("full", "valid"):
        want = lconv_want(xh, hh, mode)
        ref = fx.LinearConv(lx, k, real, mode, real_data, 0)
        assert ref.describe().startswith("lconv overlap-save: block 2048 "), ref.describe()
        ref.set_filters(h)
        y = {1: ref.apply(x)}
        t = 3 * base_tol(ref.describe(), real)
        err = rel_l2(y[1].cpu().numpy(), want)
        print(f"lconv chunks {real} {'real' if real_data else 'complex'} {mode}: unchunked err {err:.3g} tol {t:.3g}  [{ref.describe()}]")
        assert err <= t, (real, real_data, mode, err)
        ref.set_option("overlap_save", 0)
        assert ref.describe().startswith("lconv padded: M=8192, "), ref.describe()
        ref.set_filters(h)
        y[0] = ref.apply(x)
        assert rel_l2(y[0].cpu().numpy(), want) <= t
        for rows in (1, 2):
            # overlap-save: rows of the bank's scratch, 2048 complex values; padded: rows of M values of the handle's kind
            for overlap_save, per in ((1, 2048 * elem(real)), (0, 8192 * (elem(real) // 2 if real_data else elem(real)))):
                def make():
                    p = fx.LinearConv(lx, k, real, mode, real_data, 0)
                    p.set_option("overlap_save", overlap_save)  # the padded route's inner handle is created here, under the bound too
                    return p
                small = bounded(monkeypatch, make, **{CONV: rows * per})
                assert (F > rows or rows == 2) if overlap_save else batch > rows
                small.set_filters(h)
                out = Guarded(torch, (batch, small.out_length()), dt)
                small.apply(x, out=out.out)
                got = out.checked()
                err = rel_l2(got.cpu().numpy(), want)
                assert err <= t, (real, real_data, mode, rows, overlap_save, err, small.describe())
                assert same_bits(torch, got, y[overlap_save]), (real, real_data, mode, rows, overlap_save, small.describe())
    assert np.array_equal(x.cpu().numpy(), xh) and np.array_equal(h.cpu().numpy(), hh)


# ---- N-dimensional real transforms and the axis plan's transpose route
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_rfftn(torch, fx, monkeypatch, real):
    """Five items of shape (12, 10, 16): the packed route, scratch bytes per item 12 * 10 rows of 16 / 2 complex values.  One item and
    two items per chunk: five and three chunks."""
    shape, batch = (12, 10, 16), 5
    per = 12 * 10 * 8 * elem(real)
    g = torch.Generator(device="cuda").manual_seed(81)
    x = torch.randn(batch, *shape, dtype=rdt(torch, real), device="cuda", generator=g)
    half = (batch, 12, 10, 9)
    t = 3e-6 if real == "f32" else 1e-12  # tests/test_gpu_realnd.py's tol() at rank 3
    ref = fx.RealFftN(shape, real, 0)
    assert ref.describe().startswith("realnd packed: "), ref.describe()
    stream = torch.cuda.current_stream().cuda_stream
    X = torch.empty(half, dtype=cdt(torch, real), device="cuda")
    ref.forward_batch_ptr(x.data_ptr(), X.data_ptr(), batch, stream=stream)
    want_X = np.fft.rfftn(x.cpu().numpy().astype(np.float64), axes=(1, 2, 3))
    y = torch.empty_like(x)
    ref.inverse_batch_ptr(X.data_ptr(), y.data_ptr(), batch, stream=stream)
    want_y = np.fft.irfftn(X.cpu().numpy().astype(np.complex128), s=shape, axes=(1, 2, 3))
    ef, ei = rel_l2(X.cpu().numpy(), want_X), rel_l2(y.cpu().numpy(), want_y)
    print(f"rfftn chunks {real}: unchunked forward err {ef:.3g} inverse err {ei:.3g} tol {t:.3g}  [{ref.describe()}]")
    assert ef <= t and ei <= t, (real, ef, ei)
    for items in (1, 2):
        small = bounded(monkeypatch, lambda: fx.RealFftN(shape, real, 0), **{REALND: items * per})
        assert small.describe() == ref.describe() and batch > items
        out = Guarded(torch, half, cdt(torch, real))
        small.forward_batch_ptr(x.data_ptr(), out.out.data_ptr(), batch, stream=stream)
        got = out.checked()
        assert rel_l2(got.cpu().numpy(), want_X) <= t, (real, items)
        assert same_bits(torch, got, X), ("forward", real, items)
        out = Guarded(torch, (batch,) + shape, rdt(torch, real))
        small.inverse_batch_ptr(X.data_ptr(), out.out.data_ptr(), batch, stream=stream)
        got = out.checked()
        assert rel_l2(got.cpu().numpy(), want_y) <= t, (real, items)
        assert torch.equal(got, y), ("inverse", real, items)


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_axis_transpose_route(torch, fx, monkeypatch, real):
    """[3, 96, 40] along axis 1 on the forced transpose route.  A bound of seven columns of 96 values: one block (40 columns) is larger
    than the scratch, so every block goes in column ranges of seven, the last one of five; a bound of one block: three chunks of whole
    blocks."""
    n, inner, outer = 96, 40, 3
    g = torch.Generator(device="cuda").manual_seed(91)
    x = randn(torch, g, (outer, n, inner), cdt(torch, real))
    create = fx.create_fft_f32 if real == "f32" else fx.create_fft_f64
    ref = bounded(monkeypatch, lambda: create(n, 0), FOURIER_AXIS_ROUTE="transpose")
    assert ref.describe_axis(inner).startswith("axis transpose: "), ref.describe_axis(inner)
    t = base_tol(ref.describe(), real) if real == "f32" else (1e-11 if "bluestein" in ref.describe() else 1e-12)  # test_gpu_axis.py's tol()
    stream = torch.cuda.current_stream().cuda_stream
    for cap, chunks in ((7 * n * elem(real), outer * 6), (n * inner * elem(real), outer)):
        small = bounded(monkeypatch, lambda: create(n, 0), FOURIER_AXIS_ROUTE="transpose", **{AXIS: cap})
        assert small.describe_axis(inner) == ref.describe_axis(inner) and chunks > 1
        for code, want in ((fx.Transform.Fft, np.fft.fft(x.cpu().numpy().astype(np.complex128), axis=1)),
                           (fx.Transform.Ifft, np.fft.ifft(x.cpu().numpy().astype(np.complex128), axis=1))):
            y = torch.empty_like(x)
            ref.transform_axis_ptr(x.data_ptr(), y.data_ptr(), outer, inner, code, stream)
            out = Guarded(torch, (outer, n, inner), cdt(torch, real))
            small.transform_axis_ptr(x.data_ptr(), out.out.data_ptr(), outer, inner, code, stream)
            got = out.checked()
            err = rel_l2(got.cpu().numpy(), want)
            print(f"axis chunks {real} cap={cap} {code.name}: err {err:.3g} tol {t:.3g}  [{ref.describe_axis(inner)}]")
            assert err <= t and rel_l2(y.cpu().numpy(), want) <= t, (real, cap, code, err)
            assert same_bits(torch, got, y), (real, cap, code)
            z = x.clone()
            small.transform_axis_ptr(z.data_ptr(), z.data_ptr(), outer, inner, code, stream)
            assert same_bits(torch, z, y), ("in place", real, cap, code)
