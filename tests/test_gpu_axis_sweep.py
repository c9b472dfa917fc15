"""Every strided-axis kernel, route edge and launch split on the MI355X (-m gpu): tests/axis_cases.py through the product library.
  lane         all 64 axis_lane_kernel<T, N> instantiations, four (inner, outer) each, against the long-double DFT matrix
  column tile  fft_pass_kernel<T, N, CG, MODE_LAST> at every N of the route, the route edges around the narrowest tile, grids of 1, 3 and
               11 workgroups, against numpy in f64 and the long-double matrix on sampled columns
  transpose    bit-equal to permute, the plan's own batched transform, permute back, at ragged 32 x 32 tile edges
  large cases  (f32, one test each) the transpose route's column ranges and row bands under the product library's own bounds, both
               launch splits of the lane route, the column tile at the route's 2^31-byte lane-offset bound
  fftn         several routes in one call
The CPU twin is tests/test_axis_sweep_emu.py.  Every test prints its worst figures: profiles/axis_sweep/gpu_test.log is a committed run."""
import numpy as np
import pytest

import axis_cases as ac
from helpers import max_rel, rel_l2
from test_gpu_chunks import Guarded, same_bits

pytestmark = pytest.mark.gpu

GIB = 1 << 30
EPS32 = float(np.finfo(np.float32).eps)


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


class DeviceSignal:
    def __init__(self, dev):
        self.dev, self.kept, self.host = dev, dev.clone(), dev.cpu().numpy()


class DeviceApi:
    """the adapter of the product library: torch tensors on cuda:0 through Fft.transform_axis, results as numpy"""

    def __init__(self, torch, fa):
        self.torch, self.fa = torch, fa

    def plan(self, real, n):
        return (self.fa.create_fft_f32 if real == "f32" else self.fa.create_fft_f64)(n, 0)

    def cdt(self, real):
        return self.torch.complex64 if real == "f32" else self.torch.complex128

    def signal(self, real, shape, seed):
        gen = self.torch.Generator(device="cuda:0").manual_seed(seed)
        return DeviceSignal(self.torch.randn(*shape, dtype=self.cdt(real), device="cuda:0", generator=gen))

    def bits(self, a, b):
        return same_bits(self.torch, a, b)

    def axis(self, plan, sig, code):
        """the out-of-place call into NaNs between sentinel bands (Guarded): bands and input bit-unchanged afterwards; the result as numpy"""
        out = Guarded(self.torch, tuple(sig.dev.shape), sig.dev.dtype)
        plan.transform_axis(sig.dev, out.out, code, 1)
        self.last = out.checked()
        assert self.bits(sig.dev, sig.kept), "the input of an out-of-place call was written"
        return self.last.cpu().numpy()

    def in_place_same_bits(self, plan, sig, code):
        z = sig.dev.clone()
        plan.transform_axis(z, z, code, 1)
        return self.bits(z, self.last)

    def permuted_batch_same_bits(self, plan, sig, code):
        outer, n, inner = sig.dev.shape
        rows = sig.dev.permute(0, 2, 1).contiguous()
        plan.transform_batch_ptr(rows.data_ptr(), rows.data_ptr(), outer * inner, code, self.torch.cuda.current_stream().cuda_stream)
        return self.bits(rows.permute(0, 2, 1).contiguous(), self.last)


@pytest.fixture
def api(torch, fa):
    return DeviceApi(torch, fa)


# ---- small cases
@pytest.mark.parametrize("part", range(ac.LANE_PARTS))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_lane_kernels(api, real, part):
    """axis_lane_kernel<T, N> for N = part + 1, part + 5, ... 32: inner 2, 63, 65 and 300, five codes, out of place between guard bands
    and in place, against the long-double DFT matrix within the bounds of a one-launch register kernel"""
    assert ac.lane_cases(api, real, part).calls == 8 * len(ac.LANE_SHAPES) * 5


@pytest.mark.parametrize("which", range(3), ids=["narrowest", "twice", "4096"])
@pytest.mark.parametrize("n", ac.COLUMN_N)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_column_tile(api, real, n, which):
    """the MODE_LAST pass of length n as a column-tile transform: the route edges around the narrowest tile, then inner = that tile, twice
    it and 4096 at outer 1, 3 and 11, within the tile-pass bounds"""
    assert ac.column_cases(api, real, n, which).calls > 0


@pytest.mark.parametrize("part", range(ac.TRANSPOSE_PARTS))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_transpose_route_bit_for_bit(api, real, part):
    assert ac.transpose_cases(api, real, part).calls == 5 * 5


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fftn_through_several_routes(torch, fa, api, real):
    """lane, transpose, rows and column tile, column tile, rows in one fftn call each, against numpy's fftn / ifftn in f64 at twice the
    tile-pass bounds"""
    worst = ac.Worst(f"fftn {real}")
    for shape, dims, steps in ac.FFTN_CASES:
        for n, inner, route in steps:
            plan = api.plan(real, n)
            assert plan.describe_axis(inner).startswith(route) and (route or plan.describe_axis(inner) == plan.describe()), (n, inner)
        sig = api.signal(real, shape, 17 + shape[1])
        for code in ac.CODES:
            y = fa.fftn(sig.dev, dims, code)
            worst.check(y.cpu().numpy(), ac.truth_fftn(sig.host, code, dims), 2 * ac.TILE_L2[real], (shape, dims, code))
            z = sig.dev.clone()
            assert fa.fftn(z, dims, code, out=z) is z
            assert api.bits(z, y), ("in place differs", real, shape, code)
        assert api.bits(sig.dev, sig.kept)
    worst.report(2 * ac.TILE_L2[real])


# ---- large cases: f32, one allocation, one call, an on-device check each; every test frees its tensors
def room_for(torch, need_bytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * need_bytes:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, this case needs 1.5 x {need_bytes / GIB:.1f} GiB")


def fill_randn(torch, x, seed):
    """standard normal values into a contiguous complex64 tensor of any size, 2^28 elements at a time"""
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    flat = torch.view_as_real(x).view(-1)
    for i0 in range(0, flat.numel(), 1 << 29):
        part = flat[i0:i0 + (1 << 29)]
        part.copy_(torch.randn(part.numel(), dtype=torch.float32, device="cuda:0", generator=gen))


def transpose_large(torch, fa, inner, walk):
    """N = 4096 along axis 1 of [1][4096][inner]: the walk axis_plan.h's constants give is the one the case claims; the whole array is
    bit-equal, on the device, to permute, the plan's batched in-place transform of the inner rows, permute back; 16 sampled columns
    against numpy within the plan's tolerance"""
    n = 4096
    assert ac.transpose_walk(n, inner, 8) == walk, ac.transpose_walk(n, inner, 8)
    block = n * inner * 8
    room_for(torch, 5 * block + ac.plan_constants()["scratch"])
    plan = fa.create_fft_f32(n, 0)
    assert plan.describe_axis(inner) == "axis transpose: " + plan.describe()
    x = torch.empty(1, n, inner, dtype=torch.complex64, device="cuda:0")
    fill_randn(torch, x, 31 + inner)
    y = torch.empty_like(x)
    plan.transform_axis(x, y, fa.Transform.Fft, 1)
    ref = x.permute(0, 2, 1).contiguous()
    plan.transform_batch_ptr(ref.data_ptr(), ref.data_ptr(), inner, fa.Transform.Fft, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same = torch.equal(torch.view_as_real(y).permute(0, 2, 1, 3), torch.view_as_real(ref))
    cols = torch.cat([torch.tensor([0, 32767, 32768, inner - 1]), torch.linspace(1, inner - 2, 12).long()]).to("cuda:0")
    got = y[0][:, cols].cpu().numpy()
    want = np.fft.fft(x[0][:, cols].cpu().numpy().astype(np.complex128), axis=0)
    del x, y, ref, plan
    torch.cuda.empty_cache()
    l2, mx, t = rel_l2(got, want), max_rel(got, want), ac.plan_tol("", "f32")
    print(f"\naxis_sweep large transpose inner={inner}: column ranges and row bands {walk}; whole array bit-equal to the permuted batched "
          f"transform: {same}; 16 columns against numpy rel_l2 {l2:.3g} max_rel {mx:.3g} (bounds {t:.3g} / {2 * t:.3g})")
    assert same, ("not the permuted batched transform", inner)
    assert l2 <= t and mx <= 2 * t, (inner, l2, mx)


def test_transpose_column_ranges_under_the_product_bound(torch, fa):
    """one block of 1.0 GiB against the 1 GiB scratch: two column ranges, 32768 + 32 columns, one row band each"""
    transpose_large(torch, fa, 32800, [(32768, [4096]), (32, [4096])])


def test_transpose_row_bands(torch, fa):
    """one block of 2.0 GiB: a column range of 32768 columns spans more than one launch's 2^31 - 1 bytes of the user array, so it goes
    in two row bands, 4092 + 4 rows (the last range, 64 columns: 4093 + 3)"""
    transpose_large(torch, fa, 65600, [(32768, [4092, 4]), (32768, [4092, 4]), (64, [4093, 3])])


def lane_large(torch, fa, inner, outer, walk):
    """N = 2 in place on [outer][2][inner]: the launches run_lane cuts the call into are the ones the case claims; the whole array, on
    the device and in slabs, against x0 + x1 and x0 - x1 formed by torch from a kept copy, within 4 eps max|x| (a range that no launch
    wrote stays O(1) off)"""
    assert ac.lane_walk(inner, outer) == walk, ac.lane_walk(inner, outer)
    assert all(nb * cw < (1 << 30) + 1 for nb, cw in walk)
    total = outer * 2 * inner * 8
    room_for(torch, 2 * total + 4 * GIB)
    plan = fa.create_fft_f32(2, 0)
    assert plan.describe_axis(inner) == "axis lane: 2"
    x = torch.empty(outer, 2, inner, dtype=torch.complex64, device="cuda:0")
    fill_randn(torch, x, 41 + outer)
    keep = x.clone()
    plan.transform_axis(x, x, fa.Transform.Fft, 1)
    torch.cuda.synchronize()
    err = torch.zeros((), dtype=torch.float32, device="cuda:0")
    top = torch.zeros((), dtype=torch.float32, device="cuda:0")
    step_o = max(1, (1 << 27) // inner)
    for o0 in range(0, outer, step_o):
        for c0 in range(0, inner, 1 << 27):
            k, g = keep[o0:o0 + step_o, :, c0:c0 + (1 << 27)], x[o0:o0 + step_o, :, c0:c0 + (1 << 27)]
            err = torch.maximum(err, (g[:, 0] - (k[:, 0] + k[:, 1])).abs().max())
            err = torch.maximum(err, (g[:, 1] - (k[:, 0] - k[:, 1])).abs().max())
            top = torch.maximum(top, k.abs().max())
    err, top = float(err), float(top)
    del x, keep, k, g
    torch.cuda.empty_cache()
    print(f"\naxis_sweep large lane inner={inner} outer={outer}: launches (blocks, columns) {walk}; largest error {err:.3g}, "
          f"bound 4 eps max|x| = {4 * EPS32 * top:.3g}")
    assert top > 1 and err <= 4 * EPS32 * top, (inner, outer, err, top)


def test_lane_column_split(torch, fa):
    """16 GiB: more than 2^30 columns in one outer block go in two launches, 2^30 and 96 columns"""
    lane_large(torch, fa, (1 << 30) + 96, 1, [(1, 1 << 30), (1, 96)])


def test_lane_outer_split(torch, fa):
    """about 17 GB: floor(2^30 / 1000003) = 1073 whole outer blocks a launch, so 1074 blocks go in launches of 1073 and 1"""
    lane_large(torch, fa, 1000003, 1074, [(1073, 1000003), (1, 1000003)])


def test_column_tile_at_its_lane_offset_bound(torch, fa):
    """N = 64, inner = 2^26 in place (32 GiB): (N / 16) * inner * 8 is exactly the 2^31 bytes the route grants the kernel's 32-bit lane
    offsets; twice that inner takes the transpose route (description only).  64 sampled columns -- the first, the last, either side of
    every multiple of 2^24 -- against numpy in f64 within the tile-pass bounds.  Beyond that, every column's DC output against torch's
    own sum of the column taken before the call: both sums are within 63 u sum|x_j| of the exact one (63 additions, u = eps / 2), so
    they differ by at most 63 eps sum|x_j|; a tile that was dropped anywhere in the array shows there."""
    n, inner = 64, 1 << 26
    plan = fa.create_fft_f32(n, 0)
    assert (n // 16) * inner * 8 == 1 << 31
    assert plan.describe_axis(inner) == "axis column tile: L=64"
    assert plan.describe_axis(2 * inner) == "axis transpose: " + plan.describe()
    room_for(torch, n * inner * 8 + 6 * GIB)
    x = torch.empty(1, n, inner, dtype=torch.complex64, device="cuda:0")
    fill_randn(torch, x, 51)
    picks = {0, inner - 1} | {m * (1 << 24) + d for m in range(1, inner >> 24) for d in (-1, 0)}
    picks |= {int(v) for v in np.linspace(1, inner - 2, 64 - len(picks))}
    assert len(picks) == 64
    cols = torch.tensor(sorted(picks)).to("cuda:0")
    before = x[0][:, cols].cpu().numpy().astype(np.complex128)
    dc = torch.empty(inner, dtype=torch.complex64, device="cuda:0")
    mass = torch.empty(inner, dtype=torch.float32, device="cuda:0")
    for c0 in range(0, inner, 1 << 22):
        dc[c0:c0 + (1 << 22)] = x[0][:, c0:c0 + (1 << 22)].sum(0)
        mass[c0:c0 + (1 << 22)] = x[0][:, c0:c0 + (1 << 22)].abs().sum(0)
    plan.transform_axis(x, x, fa.Transform.Fft, 1)
    torch.cuda.synchronize()
    after = x[0][:, cols].cpu().numpy()
    ratio = float(((x[0, 0] - dc).abs() / mass).max())
    del x, dc, mass
    torch.cuda.empty_cache()
    want = np.fft.fft(before, axis=0)
    l2, mx, t = rel_l2(after, want), max_rel(after, want), ac.TILE_L2["f32"]
    print(f"\naxis_sweep large column tile N=64 inner=2^26: 64 columns against numpy rel_l2 {l2:.3g} max_rel {mx:.3g} (bounds {t:.3g} / "
          f"{2 * t:.3g}); DC row of all 2^26 columns: largest |y0 - sum x_j| / sum|x_j| {ratio:.3g} (bound 63 eps = {63 * EPS32:.3g})")
    assert l2 <= t and mx <= 2 * t, (l2, mx)
    assert ratio <= 63 * EPS32, ratio
