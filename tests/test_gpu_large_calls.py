"""Calls beyond 2^32 bytes through the product library on the MI355X (-m gpu, f32 on the routes named beside each test, asserted with
describe()).  The one-launch and fused routes take a call whole and address the caller's arrays with 64-bit expressions of 32-bit
row, frame and lane indices; the composed routes walk chunks at host offsets such as in + b0 * n; the resampling handle's remap and
the real plan's untangle split a chunk into launches of at most 2^31 - 1 bytes.  Below 2^32 bytes -- all that the rest of the suite
hands to a handle -- a missing cast or a wrong pointer step gives correct results.  Every case here is sized so that its largest array
lies a few rows past 2^32 bytes; the row lengths are small and the batch makes the size.

Every call is checked by three independent oracles (large_call):
  1. the same handle called on slabs of whole rows, each array of a slab below 2^31 bytes from the slab's own base (the regime the
     rest of the suite validates), into a slab-sized temporary: bit-equal to the matching slice of the large call's output, slab by
     slab on the device.  Any index that wraps in the large call breaks equality somewhere.  Where a slab starts matters: the row
     kernels of the complex plan (n <= 1024) run several transforms in a workgroup, and the last bit of about a tenth of a row's values
     depends on whether the row is an even or an odd one of its exec call -- a batched transform that starts one row later differs by
     half an ulp here and there, one that starts two rows later is bit-equal (seen at batches of 9 and of 70000 alike: arithmetic, not
     addressing).  So slabs start on multiples of 1024 rows, and where a handle walks chunks of its own the slabs start on its chunk
     boundaries (chunk_rows_of), so that every inner transform keeps its place in its exec call.
  2. the f64 truth on sampled rows -- the first and the last, the rows on either side of byte offsets 2^31 and 2^32 and of element
     offsets 2^31 and 2^32 (where reached) of every input and of the output, a dozen spread evenly -- under the tolerance of the
     handle's own GPU test (restated in tests/launch_cases.py: base() and its multiples).  This pins the slabs to the truth.
  3. the whole array on the device: the output is prefilled with NaN and none may be left; the guard elements on either side of it are
     intact; the inputs' sampled rows are unchanged; and where the case has an inverse the round trip over the WHOLE array, under the
     tolerance of the handle's own round-trip test (Hilbert: Re z == x).
Every figure is printed with its bound before it is asserted.  profiles/launch_splits/gpu_test.log is a committed run: no case skips."""
import ctypes
import math
import os

import numpy as np
import pytest

import bandspec_truth
import csd_truth
import czt_truth
import hilbert_truth
import ipfb_truth
import launch_cases as cases
import mdct_truth
import pfb_truth
import r2r_truth
import resample_truth
import spectrogram_truth
import stft_truth
import xcorr_truth
from helpers import rel_l2

pytestmark = pytest.mark.gpu

GIB = 1 << 30
PAST = 1 << 32                      # what the largest array of every case lies just past
GUARD = 64
SENTINEL = 77.0
SLAB_BYTES = (1 << 31) - 1
REAL_LAUNCH_BYTES = (1 << 31) - 1   # real_plan.h
REAL_SCRATCH_BYTES = 1 << 30        # real_plan.h: the product's scratch bound


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
    cases.print_worst()


def room_for(torch, need_bytes):
    """tests/test_gpu_axis_sweep.py's: skip where the device has less than 1.5 x the case's arrays free (a 288 GB device never does)"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * need_bytes:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, this case needs 1.5 x {need_bytes / GIB:.1f} GiB")


def fill_randn(torch, x, seed):
    """tests/test_gpu_axis_sweep.py's, for any floating or complex dtype: standard normal values into a contiguous tensor of any size,
    2^28 values at a time"""
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    flat = (torch.view_as_real(x) if x.is_complex() else x).view(-1)
    for i0 in range(0, flat.numel(), 1 << 28):
        part = flat[i0:i0 + (1 << 28)]
        part.copy_(torch.randn(part.numel(), dtype=flat.dtype, device="cuda:0", generator=gen))


def past_4_gib(row_bytes, extra=3):
    """the smallest batch whose rows of `row_bytes` pass 2^32 bytes, and three more rows"""
    return -(-PAST // row_bytes) + extra


def row_bytes(t):
    return t[0].numel() * t.element_size()


def randn_rows(torch, batch, shape, dtype, seed):
    x = torch.empty(batch, *shape, dtype=dtype, device="cuda:0")
    fill_randn(torch, x, seed)
    return x


def guarded(torch, batch, shape, dtype):
    """(buffer, output): `batch` rows of `shape` prefilled with NaN, between GUARD sentinel elements in one allocation"""
    count = batch * int(np.prod(shape))
    buf = torch.empty(count + 2 * GUARD, dtype=dtype, device="cuda:0")
    buf[:GUARD] = SENTINEL
    buf[-GUARD:] = SENTINEL
    out = buf[GUARD:GUARD + count].view(batch, *shape)
    out.fill_(float("nan"))
    return buf, out


def guards_intact(buf):
    lo, hi = buf[:GUARD].cpu().numpy(), buf[-GUARD:].cpu().numpy()
    return bool(np.all(lo == SENTINEL) and np.all(hi == SENTINEL))


def bits(torch, t):
    return torch.view_as_real(t) if t.is_complex() else t


def sample_rows(batch, arrays):
    """the rows of oracle 2 for arrays of `batch` rows: `arrays` holds (bytes per row, real or complex values per row)"""
    rows = {0, batch - 1} | {int(r) for r in np.linspace(0, batch - 1, 12)}
    for per_bytes, per_values in arrays:
        for offset in (1 << 31, 1 << 32):
            for unit in (per_bytes, per_values):
                r = offset // unit
                rows |= {r - 1, r, r + 1}
    return sorted(r for r in rows if 0 <= r < batch)


def large_call(torch, family, what, describe, ins, out_shape, out_dtype, call, truth, factor=None, err=None, bound=None, unit=1, real="f32",
               with_rows=False, align=1024):
    """One large call under the three oracles.  ins: the input tensors, `batch` rows each; call(pointers of the inputs' first rows,
    pointer of the output's first row, rows, index of the first row in the large call) enqueues the entry point on the current
    stream; truth(host rows of every input) is the f64 result of those rows.  The figure is the relative L2 error over the sampled
    rows within factor x base(), or err(got, want) within `bound`.  `unit`: slabs start on multiples of it (the filter of a row counts
    from the call's first row) and of `align` (see the module's text: 1024, or the rows of the handle's own chunk); with_rows:
    truth(sampled row indices, host rows ...).  Returns (guard buffer, output)."""
    batch = ins[0].shape[0]
    buf, out = guarded(torch, batch, out_shape, out_dtype)
    arrays = [(row_bytes(t), t[0].numel()) for t in ins + [out]]
    rows = sample_rows(batch, arrays)
    kept = [t[rows].cpu().numpy() for t in ins]
    largest = max(per * batch for per, _ in arrays)
    assert largest > PAST, (what, largest)
    call([t.data_ptr() for t in ins], out.data_ptr(), batch, 0)
    # 1. slabs of whole rows, every array of a slab below 2^31 bytes; 3. no NaN left
    step = unit * align // math.gcd(unit, align)
    slab = min(SLAB_BYTES // per for per, _ in arrays) // step * step
    assert 0 < slab < batch
    tmp = torch.empty(slab, *out_shape, dtype=out_dtype, device="cuda:0")
    for r0 in range(0, batch, slab):
        nr = min(slab, batch - r0)
        part = tmp[:nr]
        part.fill_(float("nan"))
        call([t[r0].data_ptr() for t in ins], part.data_ptr(), nr, r0)
        assert not bool(torch.isnan(bits(torch, out[r0:r0 + nr])).any()), (family, what, "a NaN of the prefill is left in rows", r0, r0 + nr)
        assert torch.equal(bits(torch, part), bits(torch, out[r0:r0 + nr])), (family, what, "the large call differs from the slab call in rows", r0, r0 + nr)
    del tmp
    print(f"large {family} {what}: {batch} rows, largest array {largest / GIB:.4f} GiB, bit-equal to {-(-batch // slab)} slab calls of {slab} rows  [{describe}]")
    # 2. the truth on sampled rows
    want = truth(rows, *kept) if with_rows else truth(*kept)
    got = out[rows].cpu().numpy()
    if err is None:
        err, bound = rel_l2, factor * cases.base(describe, real)
    cases.figure(family, real, f"large {what}, {len(rows)} sampled rows", err(got, want), bound)
    # 3. guards, inputs
    assert guards_intact(buf), (family, what, "a guard element was written")
    for t, k in zip(ins, kept):
        assert np.array_equal(t[rows].cpu().numpy(), k), (family, what, "an input was modified")
    return buf, out


def chunk_rows_of(per_row, scratch_per_item):
    """rows of a chunk of a composed inverse route under the product's scratch bound: whole rows of `per_row` items (frames) of
    `scratch_per_item` bytes each (frame_inverse_chunks, frame_plan_common.h)"""
    return REAL_SCRATCH_BYTES // scratch_per_item // per_row


def whole_rel_l2(torch, got, want, row_wise=False):
    """the relative L2 error of `got` against `want` over whole arrays of rows, accumulated in f64 on the device a few rows at a time;
    row_wise: the largest of the rows' own errors"""
    batch = got.shape[0]
    step = max(1, (1 << 26) // max(1, got[0].numel()))
    num = torch.zeros((), dtype=torch.float64, device="cuda:0")
    den = torch.zeros((), dtype=torch.float64, device="cuda:0")
    worst = 0.0
    for r0 in range(0, batch, step):
        nr = min(step, batch - r0)
        a, b = bits(torch, got[r0:r0 + nr]).double().reshape(nr, -1), bits(torch, want[r0:r0 + nr]).double().reshape(nr, -1)
        d2, b2 = (a - b).pow(2).sum(dim=1), b.pow(2).sum(dim=1)
        if row_wise:
            worst = max(worst, float((d2 / b2).sqrt().max()))
        num += d2.sum()
        den += b2.sum()
    return worst if row_wise else float((num / den).sqrt())


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- the fused frame routes
def test_stft_fused_forward_then_inverse(torch, fa):
    """n_fft 256, hop 64, reflect padding, a periodic Hann window, rows of 2^16 samples: 1025 frames of 129 bins a row, the output past
    2^32 bytes (stft_rows_kernel's out + g * bins over the flat frame index).  Then inverse() of that output: the composed route walks
    chunks of the product's 1 GiB scratch, in + (b0 * fr + f_lo) * bins beyond 2^32 bytes.  Round trip over the whole array within 4 x
    2e-6 (test_gpu_stft.py)."""
    n, hop, length = 256, 64, 1 << 16
    plan = fa.Stft(n, "f32", hop, None, True, "reflect")
    d = plan.describe()
    assert d.startswith("stft fused rows, istft composed: "), d
    fr, bins = plan.frames(length), plan.bins()
    assert (fr, bins) == (1025, 129)
    batch = past_4_gib(fr * bins * 8)
    room_for(torch, batch * (fr * bins * 8 + 2 * length * 4) + 3 * GIB)
    s = stream_of(torch)
    w = torch.hann_window(n, periodic=True, dtype=torch.float32, device="cuda:0")
    wh = w.cpu().numpy()
    plan.set_window_ptr(w.data_ptr(), s)
    x = randn_rows(torch, batch, (length,), torch.float32, 1)
    bufX, X = large_call(torch, "stft", "forward", d, [x], (fr, bins), torch.complex64,
                         lambda i, o, nb, b0: plan.forward_ptr(i[0], o, length, nb, False, s),
                         lambda xh: stft_truth.stft(xh, n, hop, n, wh, "reflect"), 2)
    chunk = chunk_rows_of(fr, n * 4)  # a frame takes n_fft reals of the scratch: 1023 rows, an ODD number of frames, a chunk
    assert chunk == 1023
    bufy, y = large_call(torch, "stft", "inverse", d, [X], (length,), torch.float32,
                         lambda i, o, nb, b0: plan.inverse_ptr(i[0], o, fr, length, nb, False, s),
                         lambda Xh: stft_truth.istft(Xh, n, hop, length, None, wh, "reflect"), 4, align=chunk)
    cases.figure("stft", "f32", "large round trip, whole array", whole_rel_l2(torch, y, x), 4 * 2e-6)


def spectrogram_plan(torch, fa, cls, n, hop, *more):
    plan = cls(n, *more, "f32", hop, None, True, "reflect")
    plan.set_option("fusion", 1)
    w = torch.hann_window(n, periodic=True, dtype=torch.float32, device="cuda:0")
    plan.set_window_ptr(w.data_ptr(), stream_of(torch))
    return plan, w.cpu().numpy()


def test_spectrogram_fused_forward(torch, fa):
    """spectrogram_rows_kernel ("fusion" = 1), power: rows of 2^16 samples, the real output of 1025 x 129 values a row past 2^32 bytes"""
    n, hop, length = 256, 64, 1 << 16
    plan, wh = spectrogram_plan(torch, fa, fa.Spectrogram, n, hop)
    d = plan.describe()
    assert d.startswith("spectrogram fused rows, welch fused rows: "), d
    fr, bins = plan.frames(length), plan.bins()
    batch = past_4_gib(fr * bins * 4)
    room_for(torch, batch * (fr * bins * 4 + length * 4) + 2 * GIB)
    s = stream_of(torch)
    x = randn_rows(torch, batch, (length,), torch.float32, 2)
    large_call(torch, "spectrogram", "forward power", d, [x], (fr, bins), torch.float32,
               lambda i, o, nb, b0: plan.forward_ptr(i[0], o, length, nb, 2, False, s),
               lambda xh: spectrogram_truth.spectrogram(xh, n, hop, n, wh, "reflect", 2, False), 4)


@pytest.mark.parametrize("past", [1, 4], ids=["2^32 bytes", "2^32 elements"])
def test_welch_fused(torch, fa, past):
    """the fused Welch average: an input of rows of 2^16 samples past 2^32 bytes (in + b0 * length of every row group, and the kernel's
    row * length).  And past 2^32 ELEMENTS, 16 GiB: an array of 2^32 bytes holds 2^30 reals, so a product of two 32-bit indices that
    lacks its cast still fits there; the Welch average, whose output is a row of bins per input row, is where passing 2^32 elements
    costs least."""
    n, hop, length = 256, 64, 1 << 16
    plan, wh = spectrogram_plan(torch, fa, fa.Spectrogram, n, hop)
    d = plan.describe()
    assert d.startswith("spectrogram fused rows, welch fused rows: "), d
    batch = past_4_gib(length * 4 // past)
    assert batch * length * 4 > past * PAST and (past == 1 or PAST < 1 << 32 or batch * length > 1 << 32)
    room_for(torch, batch * length * 4 + 3 * GIB)
    s = stream_of(torch)
    x = randn_rows(torch, batch, (length,), torch.float32, 3)
    large_call(torch, "welch", f"welch, {batch * length * 4 / GIB:.1f} GiB", d, [x], (plan.bins(),), torch.float32,
               lambda i, o, nb, b0: plan.welch_ptr(i[0], o, length, nb, True, 0.37, s),
               lambda xh: spectrogram_truth.welch(xh, n, hop, n, wh, "reflect", True, 0.37), 4)


def test_csd_fused(torch, fa):
    """the fused cross spectrum: x and y of rows of 2^16 samples, past 2^32 bytes each.  Bound: test_gpu_csd.py's 4 x base."""
    n, hop, length = 256, 64, 1 << 16
    plan, wh = spectrogram_plan(torch, fa, fa.CrossSpectrum, n, hop)
    d = plan.describe()
    assert d.startswith("csd fused rows, coherence fused rows: "), d
    batch = past_4_gib(length * 4)
    room_for(torch, 2 * batch * length * 4 + 3 * GIB)
    s = stream_of(torch)
    x, y = randn_rows(torch, batch, (length,), torch.float32, 4), randn_rows(torch, batch, (length,), torch.float32, 5)
    large_call(torch, "csd", "csd", d, [x, y], (plan.bins(),), torch.complex64,
               lambda i, o, nb, b0: plan.csd_ptr(i[0], i[1], o, length, nb, True, 0.37, s),
               lambda xh, yh: csd_truth.csd(xh, yh, n, hop, n, wh, "reflect", True, 0.37), 4)


def test_bandspec_fused(torch, fa):
    """bandspec_rows_kernel: an input of rows of 2^16 samples past 2^32 bytes, 24 signed bands.  Figure and bound: tests/bandspec_cases.py's."""
    n, hop, length, bands = 256, 64, 1 << 16, 24
    plan, wh = spectrogram_plan(torch, fa, fa.BandSpectrogram, n, hop, bands)
    d = plan.describe()
    assert d.startswith("bandspec fused rows: "), d
    W = np.ascontiguousarray(np.random.default_rng(6).standard_normal((bands, n // 2 + 1)).astype(np.float32))
    s = stream_of(torch)
    plan.set_bands_ptr(W.ctypes.data, s)
    fr = plan.frames(length)
    batch = past_4_gib(length * 4)
    room_for(torch, batch * (length * 4 + fr * bands * 4) + 3 * GIB)
    x = randn_rows(torch, batch, (length,), torch.float32, 7)
    W64 = W.astype(np.float64)
    scale = {}

    def truth(xh):
        scale["abs"] = float(np.linalg.norm(bandspec_truth.abs_band_spectrogram(xh, W64, n, hop, n, wh, "reflect", 2, False)))
        return bandspec_truth.band_spectrogram(xh, W64, n, hop, n, wh, "reflect", 2, False)
    large_call(torch, "bandspec", "forward", d, [x], (fr, bands), torch.float32,
               lambda i, o, nb, b0: plan.forward_ptr(i[0], o, length, nb, 2, False, 0.0, 0.0, s), truth,
               err=lambda got, want: float(np.linalg.norm(got - want)) / scale["abs"], bound=4 * cases.base(d, "f32"))


def test_mdct_fused_forward_then_inverse(torch, fa):
    """n = 256 coefficients a frame ("fusion" = 1), centred, the sine window, rows of 2^16 samples: input and output past 2^32 bytes;
    then the inverse, whose chunks walk the 1 GiB scratch.  Round trip over the whole array within test_gpu_mdct.py's 4 x base."""
    n, length = 256, 1 << 16
    plan = fa.Mdct(n, "f32", True)
    plan.set_option("fusion", 1)
    d = plan.describe()
    assert d.startswith("mdct fused rows, imdct composed: "), d
    fr = plan.frames(length)
    assert fr == mdct_truth.frames(length, n, True) and plan.default_length(fr) >= length
    batch = past_4_gib(length * 4)
    room_for(torch, batch * (2 * length * 4 + fr * n * 4) + 3 * GIB)
    s = stream_of(torch)
    x = randn_rows(torch, batch, (length,), torch.float32, 8)
    bufX, X = large_call(torch, "mdct", "forward", d, [x], (fr, n), torch.float32,
                         lambda i, o, nb, b0: plan.forward_ptr(i[0], o, length, nb, False, s),
                         lambda xh: mdct_truth.mdct(xh, n, None, True), 2)
    bufy, y = large_call(torch, "mdct", "inverse", d, [X], (length,), torch.float32,
                         lambda i, o, nb, b0: plan.inverse_ptr(i[0], o, fr, length, nb, False, s),
                         lambda Xh: mdct_truth.imdct(Xh, n, length, mdct_truth.sine_window(n, np.float32), True), 4,
                         align=chunk_rows_of(fr, n * 8))  # a frame takes n complex values of the scratch
    cases.figure("mdct", "f32", "large round trip, whole array", whole_rel_l2(torch, y, x), 4 * cases.base(d, "f32"))


def test_pfb_fused_forward_then_the_synthesis_bank(torch, fa):
    """256 channels, 4 taps, hop 256, real rows of 2^16 samples: pfb_rows_kernel's input past 2^32 bytes; then the synthesis bank's
    inverse of the frames to real rows of 2^16 samples, an output past 2^32 bytes (ipfb_gather_kernel's o0 = row * length + t)"""
    P, T, D, length = 256, 4, 256, 1 << 16
    ana, syn = fa.Pfb(P, T, "f32", D, True), fa.Ipfb(P, T, "f32", D, True)
    da, ds = ana.describe(), syn.describe()
    assert da.startswith("pfb fused rows: ") and ds.startswith("ipfb composed: "), (da, ds)
    fr, bins = ana.frames(length), ana.bins()
    assert fr == pfb_truth.frames(length, P, T, D) and syn.length(fr) == length and bins == P // 2 + 1
    batch = past_4_gib(length * 4)
    room_for(torch, batch * (2 * length * 4 + fr * bins * 8) + 3 * GIB)
    s = stream_of(torch)
    hh = cases.uniform(np.random.default_rng(9), "f32", P * T)
    h = torch.from_numpy(hh).cuda()
    ana.set_filter_ptr(h.data_ptr(), s)
    syn.set_filter_ptr(h.data_ptr(), s)
    x = randn_rows(torch, batch, (length,), torch.float32, 10)
    bufY, Y = large_call(torch, "pfb", "forward", da, [x], (fr, bins), torch.complex64,
                         lambda i, o, nb, b0: ana.forward_ptr(i[0], o, length, nb, s),
                         lambda xh: pfb_truth.pfb(xh, hh, P, T, D, True), 2)
    large_call(torch, "ipfb", "inverse", ds, [Y], (length,), torch.float32,
               lambda i, o, nb, b0: syn.inverse_ptr(i[0], o, fr, length, nb, s),
               lambda Yh: ipfb_truth.synth(Yh, hh, P, T, D, True, length), 2, align=chunk_rows_of(fr, P * 4))  # P reals a frame


# ---- the one-launch routes
def test_hilbert_one_launch_analytic_and_envelope(torch, fa):
    """n = 2048 ("fusion" = 1): analytic with the output past 2^32 bytes, Re z == x over the whole array within test_gpu_hilbert.py's
    2 x base; envelope with the input past 2^32 bytes"""
    n = 2048
    plan = fa.Hilbert(n, "f32")
    plan.set_option("fusion", 1)
    d = plan.describe()
    assert d.startswith("hilbert one-launch: "), d
    s = stream_of(torch)
    batch = past_4_gib(n * 8)
    room_for(torch, batch * n * 12 + 3 * GIB)
    x = randn_rows(torch, batch, (n,), torch.float32, 11)
    bufz, z = large_call(torch, "hilbert", "analytic", d, [x], (n,), torch.complex64,
                         lambda i, o, nb, b0: plan.analytic_ptr(i[0], o, nb, s), hilbert_truth.analytic, 2)
    cases.figure("hilbert", "f32", "large Re z against x, whole array", whole_rel_l2(torch, torch.view_as_real(z)[..., 0], x), 2 * cases.base(d, "f32"))
    del bufz, z, x
    batch = past_4_gib(n * 4)
    room_for(torch, batch * n * 8 + 3 * GIB)
    x = randn_rows(torch, batch, (n,), torch.float32, 12)
    large_call(torch, "hilbert", "envelope", d, [x], (n,), torch.float32,
               lambda i, o, nb, b0: plan.envelope_ptr(i[0], o, nb, s), hilbert_truth.envelope, 2)


def test_xcorr_one_launch(torch, fa):
    """L = 2048, n = 1024, the full lag window, the output past 2^32 bytes.  f64: the product ships the one-launch kernel of real rows
    at f64 without weighting only (tests/test_gpu_xcorr.py), and that instance has the addressing this case is about.  Bound:
    test_gpu_xcorr.py's 4 x base on the window error."""
    n, L = 1024, 2048
    plan = fa.CrossCorrelation(n, L, 0, L, "f64", True)
    d = plan.describe()
    assert d.startswith("xcorr one-launch: "), d
    s = stream_of(torch)
    batch = past_4_gib(L * 8)
    room_for(torch, batch * (L * 8 + 2 * n * 8) + 3 * GIB)
    x, y = randn_rows(torch, batch, (n,), torch.float64, 13), randn_rows(torch, batch, (n,), torch.float64, 14)
    large_call(torch, "xcorr", "correlate", d, [x, y], (L,), torch.float64,
               lambda i, o, nb, b0: plan.correlate_ptr(i[0], i[1], o, nb, s), lambda xh, yh: xcorr_truth.full(xh, yh, L),
               err=lambda got, want: xcorr_truth.window_err(got, want, 0, L), bound=4 * cases.base(d, "f64"), real="f64")


def test_czt_one_launch(torch, fa):
    """n = m = 1000 (L = 2048) on the unit circle: input and output past 2^32 bytes.  Bound: tests/czt_cases.py's BASE x chirp_ratio."""
    n = m = 1000
    plan = fa.Czt(n, m, real="f32")
    d = plan.describe()
    assert d.startswith("czt one-launch: "), d
    s = stream_of(torch)
    batch = past_4_gib(m * 8)
    room_for(torch, batch * (n + m) * 8 + 3 * GIB)
    x = randn_rows(torch, batch, (n,), torch.complex64, 15)
    large_call(torch, "czt", "transform", d, [x], (m,), torch.complex64, lambda i, o, nb, b0: plan.transform_ptr(i[0], o, nb, s),
               lambda xh: czt_truth.czt(xh, m, 1.0, -1.0 / m), err=rel_l2,
               bound=cases.CZT_BASE["f32"] * czt_truth.chirp_ratio(n, m, 1.0, 1.0))


def test_circular_convolution_one_launch(torch, fa):
    """complex rows of 4096 values, three filters of 33 taps: input and output past 2^32 bytes; row b takes filter b mod 3 counted from
    the call's first row, so the slabs start on multiples of 3.  tol(): test_gpu_conv.py's, 3 x base."""
    n, F, taps = 4096, 3, 33
    plan = fa.FftConv(n, "f32", False)
    s = stream_of(torch)
    hh = cases.randn(np.random.default_rng(16), (F, taps), np.complex64)
    h = torch.from_numpy(hh).cuda()
    plan.set_filters_ptr(h.data_ptr(), taps, F, False, s)
    d = plan.describe()
    assert d.startswith("conv one-launch: "), d
    batch = past_4_gib(n * 8)
    room_for(torch, 2 * batch * n * 8 + 3 * GIB)
    x = randn_rows(torch, batch, (n,), torch.complex64, 17)

    def truth(rows, xh):  # the sampled rows keep their own filters
        return np.stack([cases.conv_want(xh[i:i + 1], hh[r % F:r % F + 1])[0] for i, r in enumerate(rows)])
    large_call(torch, "conv", "apply", d, [x], (n,), torch.complex64, lambda i, o, nb, b0: plan.apply_ptr(i[0], o, nb, s), truth, 3, unit=F,
               with_rows=True)


def test_linear_convolution_overlap_save(torch, fa):
    """real rows of 5000 samples, two filters of 129 taps, mode full: lconv_small_kernel's input past 2^32 bytes; slabs start on even
    rows.  tol(): test_gpu_lconv.py's, 3 x base."""
    lx, k, F = 5000, 129, 2
    plan = fa.LinearConv(lx, k, "f32", "full", True)
    s = stream_of(torch)
    hh = cases.randn(np.random.default_rng(18), (F, k), np.float32)
    h = torch.from_numpy(hh).cuda()
    plan.set_filters_ptr(h.data_ptr(), F, False, s)
    d = plan.describe()
    assert d.startswith("lconv overlap-save: block 2048 "), d
    lout = plan.out_length()
    batch = past_4_gib(lx * 4)
    room_for(torch, batch * (lx + lout) * 4 + 3 * GIB)
    x = randn_rows(torch, batch, (lx,), torch.float32, 19)

    def truth(rows, xh):
        return np.stack([cases.lconv_want(xh[i:i + 1], hh[r % F:r % F + 1], "full")[0] for i, r in enumerate(rows)])
    large_call(torch, "lconv", "apply", d, [x], (lout,), torch.float32, lambda i, o, nb, b0: plan.apply_ptr(i[0], o, nb, s), truth, 3, unit=F,
               with_rows=True)


# ---- resampling: the split that is live in the product
def resample_walk(batch, n, m):
    """the chunks of a call of complex f32 rows and the launches of the remap in each (resample_plan.h): a chunk holds 1 GiB of input
    rows, a launch at most 2^31 - 1 bytes of the larger side"""
    chunk = cases.chunk_rows(batch, REAL_SCRATCH_BYTES, n * 8)
    return [cases.sizes(nb, max(1, REAL_LAUNCH_BYTES // (max(n, m) * 8))) for nb in cases.sizes(batch, chunk)]


@pytest.mark.parametrize("batch,walk", [(65537, [[65535, 2]]), (131075, [[65535, 65535, 2], [3]])], ids=["65537", "131075"])
def test_resample_complex_rows_split_their_remap(torch, fa, batch, walk):
    """complex rows 1024 -> 4096.  A chunk is sized by the INPUT row, the remap writes the caller's OUTPUT rows of four times that: 65537
    rows are one chunk whose output passes 2^31 bytes, in launches of 65535 and 2 rows (the first launch's largest byte offset 32 KiB
    below 2^31); 131075 rows are a chunk of 131072 rows in three launches and a chunk of 3, the output past 2^32 bytes.  The larger case
    meets all of large_call's conditions; the smaller one is checked the same way with its output past 2^31 bytes.  tol():
    test_gpu_resample.py's, 2 x base."""
    n, m = 1024, 4096
    assert resample_walk(batch, n, m) == walk
    plan = fa.Resample(n, m, "f32", real_input=False)
    d = plan.describe()
    assert d.startswith("resample complex: "), d
    s = stream_of(torch)
    room_for(torch, batch * (n + m) * 8 + 4 * GIB)
    x = randn_rows(torch, batch, (n,), torch.complex64, 20 + batch % 7)
    if batch * m * 8 > PAST:
        large_call(torch, "resample", f"complex {batch} rows", d, [x], (m,), torch.complex64,
                   lambda i, o, nb, b0: plan.forward_ptr(i[0], o, nb, s), lambda xh: resample_truth.resample(xh, m), 2)
        return
    # the output lies between 2^31 and 2^32 bytes: large_call's oracles with slabs of half the rows
    buf, out = guarded(torch, batch, (m,), torch.complex64)
    rows = sample_rows(batch, [(n * 8, n), (m * 8, m)]) + [65534, 65535, 65536]
    rows = sorted(set(rows))
    kept = x[rows].cpu().numpy()
    plan.forward_ptr(x.data_ptr(), out.data_ptr(), batch, s)
    slab = 32768
    tmp = torch.empty(slab, m, dtype=torch.complex64, device="cuda:0")
    for r0 in range(0, batch, slab):
        nr = min(slab, batch - r0)
        tmp[:nr].fill_(float("nan"))
        plan.forward_ptr(x[r0].data_ptr(), tmp.data_ptr(), nr, s)
        assert not bool(torch.isnan(bits(torch, out[r0:r0 + nr])).any()), ("a NaN of the prefill is left in rows", r0, r0 + nr)
        assert torch.equal(bits(torch, tmp[:nr]), bits(torch, out[r0:r0 + nr])), ("the large call differs from the slab call in rows", r0, r0 + nr)
    print(f"large resample complex {batch} rows: output {batch * m * 8 / GIB:.4f} GiB, bit-equal to 3 slab calls  [{d}]")
    cases.figure("resample", "f32", f"large complex {batch} rows, {len(rows)} sampled rows", rel_l2(out[rows].cpu().numpy(), resample_truth.resample(kept, m)),
                 2 * cases.base(d, "f32"))
    assert guards_intact(buf) and np.array_equal(x[rows].cpu().numpy(), kept)


def test_resample_real_rows_fused_untangle(torch, fa):
    """real rows 1024 -> 4096 on the fused untangle route: the output past 2^32 bytes, chunks of the 1 GiB scratch"""
    n, m = 1024, 4096
    plan = fa.Resample(n, m, "f32", real_input=True)
    d = plan.describe()
    assert d.startswith("resample real fused untangle: "), d
    s = stream_of(torch)
    batch = past_4_gib(m * 4)
    room_for(torch, batch * (n + m) * 4 + 4 * GIB)
    x = randn_rows(torch, batch, (n,), torch.float32, 21)
    large_call(torch, "resample", "real fused untangle", d, [x], (m,), torch.float32,
               lambda i, o, nb, b0: plan.forward_ptr(i[0], o, nb, s), lambda xh: resample_truth.resample(xh, m), 2,
               align=cases.chunk_rows(batch, REAL_SCRATCH_BYTES, (n // 2 + 1 + m // 2 + 1) * 8))  # resample_plan.h's row_bytes()


# ---- the real-input handles
def rfft_round_trip(torch, fa, plan, d, family):
    """rfft then irfft with n = 4096: input and half spectrum past 2^32 bytes; every row's round trip within 4e-6 (test_gpu_real.py)"""
    n = 4096
    s = stream_of(torch)
    batch = past_4_gib(n * 4)
    room_for(torch, batch * (2 * n * 4 + (n // 2 + 1) * 8) + 6 * GIB)
    x = randn_rows(torch, batch, (n,), torch.float32, 22)
    bufX, X = large_call(torch, family, "rfft", d, [x], (n // 2 + 1,), torch.complex64,
                         lambda i, o, nb, b0: plan.forward_batch_ptr(i[0], o, nb, fa.Transform.Fft, s),
                         lambda xh: np.fft.rfft(xh.astype(np.float64), axis=-1), 1)
    bufy, y = large_call(torch, family, "irfft", d, [X], (n,), torch.float32,
                         lambda i, o, nb, b0: plan.inverse_batch_ptr(i[0], o, nb, fa.Transform.Ifft, s),
                         lambda Xh: np.fft.irfft(Xh.astype(np.complex128), n=n, axis=-1), 1)
    cases.figure(family, "f32", "large round trip, the worst row of the whole array", whole_rel_l2(torch, y, x, row_wise=True), 4e-6)
    return batch


def test_rfft_then_irfft(torch, fa):
    plan = fa.RealFft(4096, "f32")
    d = plan.describe()
    assert d.startswith("real half-length: "), d
    rfft_round_trip(torch, fa, plan, d, "real")


def test_rfft_under_a_scratch_of_4_gib_runs_full_size_untangle_launches(torch, fa, monkeypatch):
    """The experiments library under FOURIER_REAL_SCRATCH_BYTES = 4 GiB: a chunk of 262144 rows, whose half-spectrum side of 2049 complex
    values a row passes 2^31 bytes, so RealPlan::sweep's REAL_LAUNCH_BYTES split runs at its real bound -- launches of 131008, 131008
    and 128 rows -- and a second chunk of 3 rows.  The oracles are rfft_round_trip's; the slab calls are one launch each."""
    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    n = 4096
    chunk = cases.chunk_rows(past_4_gib(n * 4), 4 * GIB, (n // 2) * 8)
    launches = cases.sizes(chunk, REAL_LAUNCH_BYTES // ((n // 2 + 1) * 8))
    assert chunk == 262144 and launches == [131008, 131008, 128] and past_4_gib(n * 4) - chunk == 3
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    try:
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(4 * GIB))
        plan = fa.RealFft(n, "f32")
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        d = plan.describe()
        assert d.startswith("real half-length: "), d
        rfft_round_trip(torch, fa, plan, d, "real 4 GiB scratch")
    finally:
        _lib._lib = prev


def test_dct_pair(torch, fa):
    """DCT-II then DCT-III, ortho, n = 4096: input and output past 2^32 bytes; the round trip over the whole array within
    test_gpu_r2r.py's 2 x tol()"""
    n = 4096
    plan = fa.R2R(n, "f32")
    d = plan.describe()
    assert d.startswith("r2r half-length: "), d
    s = stream_of(torch)
    batch = past_4_gib(n * 4)
    room_for(torch, 3 * batch * n * 4 + 4 * GIB)
    x = randn_rows(torch, batch, (n,), torch.float32, 23)
    K, ortho = r2r_truth.KINDS, r2r_truth.NORMS["ortho"]

    def truth(kind):
        def f(xh):
            idx, want = r2r_truth.want(kind, "ortho", xh)
            f.idx = idx
            return want
        return f
    t2, t3 = truth("dct2"), truth("dct3")
    bufy, y = large_call(torch, "r2r", "dct2", d, [x], (n,), torch.float32,
                         lambda i, o, nb, b0: plan.transform_batch_ptr(i[0], o, nb, K["dct2"], ortho, s), t2,
                         err=lambda got, want: rel_l2(got[:, t2.idx], want), bound=2 * cases.base(d, "f32"))
    bufz, z = large_call(torch, "r2r", "dct3", d, [y], (n,), torch.float32,
                         lambda i, o, nb, b0: plan.transform_batch_ptr(i[0], o, nb, K["dct3"], ortho, s), t3,
                         err=lambda got, want: rel_l2(got[:, t3.idx], want), bound=2 * cases.base(d, "f32"))
    cases.figure("r2r", "f32", "large round trip, whole array", whole_rel_l2(torch, z, x), 2 * 2 * cases.base(d, "f32"))


def test_rfft2_then_irfft2(torch, fa):
    """items of 64 x 64 reals: the input past 2^32 bytes in both directions (the half spectrum of 64 x 33 values an item with it); the
    round trip over the whole array within test_gpu_realnd.py's tol() at rank 2"""
    shape = (64, 64)
    plan = fa.RealFftN(shape, "f32")
    d = plan.describe()
    assert d.startswith("realnd "), d
    s = stream_of(torch)
    batch = past_4_gib(64 * 64 * 4)
    room_for(torch, batch * (2 * 64 * 64 * 4 + 64 * 33 * 8) + 4 * GIB)
    x = randn_rows(torch, batch, shape, torch.float32, 24)
    bufX, X = large_call(torch, "realnd", "rfft2", d, [x], (64, 33), torch.complex64,
                         lambda i, o, nb, b0: plan.forward_batch_ptr(i[0], o, nb, fa.Transform.Fft, s),
                         lambda xh: np.fft.rfft2(xh.astype(np.float64)), err=rel_l2, bound=2e-6)
    bufy, y = large_call(torch, "realnd", "irfft2", d, [X], shape, torch.float32,
                         lambda i, o, nb, b0: plan.inverse_batch_ptr(i[0], o, nb, fa.Transform.Ifft, s),
                         lambda Xh: np.fft.irfft2(Xh.astype(np.complex128), s=shape), err=rel_l2, bound=2e-6)
    cases.figure("realnd", "f32", "large round trip, whole array", whole_rel_l2(torch, y, x), 2e-6)
