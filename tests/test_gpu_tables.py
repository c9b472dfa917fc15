"""Every ahead-of-time kernel of the core engine's two generated tables on the GPU (-m gpu): each register-stage row of
fourier_amd/csrc/regfft_shapes.h in each precision that adopts it, and each tile-pass length of kernels_regtile.cpp / kernels_tiled.cpp in
each role a default plan gives it (plain first / last pass; Bluestein chirp-in / chirp-out and conv pass).  The other GPU tests name a few
dozen of these kernels; a row that is miscompiled, carries a variant flag its shape was never tried with, has a wrong table entry or has
silently fallen back to another route shows here.

Every call goes through `guarded`: input and output sit inside larger device buffers with at least one transform of sentinel on each
side, and the bands, the input of an out-of-place call and the in-place result are compared bit for bit.

Bounds (from the tests these kernels already have, not from this sweep): rel-L2 against numpy's FFT of the input widened to complex128
4e-7 (f32) / 3e-15 (f64) for register-stage rows (test_lengths_with_prime_factors_5_to_13_run_as_stockham_passes), 4e-7 / 4e-15 for tile
plans in both roles (test_bluestein_on_a_smooth_work_array); the largest error of one transform over the largest value of its spectrum at
most twice that (the ratio of test_pow2_all_codes_vs_oracle).  numpy's own complex64 FFT over all 834 table lengths on these inputs has
rel-L2 <= 4.4e-8 and max_rel <= 7.1e-8.  Each case prints the worst figures it saw: profiles/table_sweep/gpu_test.log is a committed run."""
import numpy as np
import pytest

import kernel_tables as kt
from helpers import hash_normal, max_rel, regfft_shape, rel_l2

pytestmark = pytest.mark.gpu

REG_L2 = {"f32": 4e-7, "f64": 3e-15}
TILE_L2 = {"f32": 4e-7, "f64": 4e-15}
DTYPE = {"f32": np.complex64, "f64": np.complex128}
FFT, SQRT_SCALED_IFFT = 0, 4  # between them: both values of the kernels' run-time arguments `swap` and `scale`


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

    _lib.lib()  # raises if the HIP library is missing: never fall back silently
    assert "fourier_amd/lib/libfourier.so" in open("/proc/self/maps").read(), "the in-tree HIP library must be the one that is loaded"
    return fourier_amd


def make(fa, n, real):
    return fa.create_fft_f32(n) if real == "f32" else fa.create_fft_f64(n)


# ---- inputs and their truth: computed once per length, shared, never written ----
_BASE = {}


def rows(n, count):
    """hash_normal(7700 + b, n) for b < count as complex128 (a pure function of seed and index: a prefix of one longer row per seed)"""
    for b in range(count):
        if b not in _BASE or _BASE[b].shape[0] < n:
            _BASE[b] = hash_normal(7700 + b, max(1 << int(n - 1).bit_length(), 32768))
            _BASE[b].setflags(write=False)
    return np.stack([_BASE[b][:n] for b in range(count)])


def inputs_and_truth(n, real, count):
    x = rows(n, count).astype(DTYPE[real])
    wide = x.astype(np.complex128)
    truth = {FFT: np.fft.fft(wide, axis=1), SQRT_SCALED_IFFT: np.fft.ifft(wide, axis=1) * np.sqrt(n)}
    return x, truth


# ---- the guarded runner ----
def _sentinel(torch, count, cdt):
    """count complex values, none of them 0, NaN or infinite, no two neighbours alike"""
    rdt = torch.float32 if cdt == torch.complex64 else torch.float64
    r = (torch.arange(2 * count, device="cuda", dtype=torch.float64) % 509 - 254.5) * 1024.0
    return torch.view_as_complex(r.to(rdt).view(count, 2))


def _bits(torch, t):
    r = torch.view_as_real(t)
    return r.view(torch.int32 if r.dtype == torch.float32 else torch.int64)


def guarded(torch, plan, x, code, inplace=False):
    """numpy (batch, n) -> the batched transform as numpy, run between two bands of sentinel of at least n elements each, in both buffers.
    Out of place: the transforms start on an ODD element (8 bytes off a 16-byte boundary in f32); input, output and every band filled with
    sentinel beforehand; afterwards the bands of both buffers and the input are bit-unchanged.  In place: bands of a multiple of 32 elements
    (the rows start on a 256-byte boundary), bit-unchanged afterwards; the caller compares the values with the out-of-place ones."""
    batch, n = x.shape
    cdt = torch.complex64 if x.dtype == np.complex64 else torch.complex128
    band = -(-n // 32) * 32 if inplace else n | 1
    lo, hi = band, band + batch * n
    src = _sentinel(torch, hi + band, cdt)
    src[lo:hi] = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
    dst = src if inplace else _sentinel(torch, hi + band, cdt)
    src_before, dst_before = _bits(torch, src).clone(), _bits(torch, dst).clone()
    e = x.dtype.itemsize
    plan.transform_batch_ptr(src.data_ptr() + lo * e, dst.data_ptr() + lo * e, batch, code)
    torch.cuda.synchronize()
    after = _bits(torch, dst)
    assert torch.equal(after[:lo], dst_before[:lo]), (plan.describe(), batch, code, inplace, "wrote below the output")
    assert torch.equal(after[hi:], dst_before[hi:]), (plan.describe(), batch, code, inplace, "wrote beyond the output")
    if not inplace:
        assert torch.equal(_bits(torch, src), src_before), (plan.describe(), batch, code, "wrote its input or the bands around it")
    return dst[lo:hi].cpu().numpy().reshape(batch, n)


class Worst:
    def __init__(self):
        self.l2 = self.mx = 0.0
        self.at_l2 = self.at_mx = None
        self.plans = 0

    def note(self, l2, mx, where):
        if l2 > self.l2:
            self.l2, self.at_l2 = l2, where
        if mx > self.mx:
            self.mx, self.at_mx = mx, where

    def report(self, what, bound):
        print(f"\ntable_sweep {what}: {self.plans} plans, worst rel_l2 {self.l2:.3g} at {self.at_l2}, worst max_rel {self.mx:.3g} at {self.at_mx}"
              f" (bounds {bound:.3g} / {2 * bound:.3g})")


def check(torch, plan, x, truth, batch, bound, worst, where):
    """`batch` rows (row b = x[b % len(x)]: equal rows land in different workgroups and must come out with equal bits), forward and
    square-root-scaled inverse, out of place and in place through the guarded runner, against the truth of the distinct rows"""
    xs = x[np.arange(batch) % x.shape[0]]
    head = min(batch, x.shape[0])
    for code in (FFT, SQRT_SCALED_IFFT):
        got = guarded(torch, plan, xs, code)
        assert np.array_equal(guarded(torch, plan, xs, code, inplace=True), got), (where, batch, code, "in place differs from out of place")
        assert all(np.array_equal(got[b], got[b % head]) for b in range(head, batch)), (where, batch, code, "equal rows, different bits")  # every workgroup
        l2 = rel_l2(got[:head], truth[code][:head])
        mx = max(max_rel(got[b], truth[code][b]) for b in range(head))
        worst.note(l2, mx, where + (batch, code))
        assert l2 <= bound and mx <= 2 * bound, (where, batch, code, l2, mx)


# ---- (a) every register-stage row ----
def _reg_cases():
    rws = [r for r in kt.regfft_rows() if not r.on_request]
    keys = sorted({(real, 3 if r.r3 else 2, kt.flag(r, real)) for r in rws for real in ("f32", "f64") if kt.flag(r, real)})
    return keys


def _reg_rows(real, stages, flag):
    return [r for r in kt.regfft_rows() if not r.on_request and kt.flag(r, real) == flag and (3 if r.r3 else 2) == stages]


def test_register_stage_cases_are_the_whole_table():
    """the cases below partition the adopted (length, precision) pairs of the default rows: the header's own 736 + 763"""
    cases = _reg_cases()
    seen = [(r.n, real) for real, stages, flag in cases for r in _reg_rows(real, stages, flag)]
    (_, f32, f64), _ = kt.regfft_counts()
    assert len(seen) == len(set(seen)) == f32 + f64 == 1499
    assert len(cases) == 12


def _reg_sweep(torch, fa, real, table_rows, worst, on_request=False):
    for r in table_rows:
        n = r.n
        plan = make(fa, n, real)
        want0 = base = None
        # two stages (N <= 900): 133 rows of 7 distinct ones are ragged against every transforms-per-workgroup count; three: 7 rows of 3 distinct
        # ones -- odd, the packed f32 pair has a lone last transform; 1: a grid of one workgroup with one transform
        x, truth = inputs_and_truth(n, real, 3 if r.r3 else 7)
        if on_request:
            base = plan.describe()
            assert "mixed-radix" in base, (n, real, base)
            want0 = guarded(torch, plan, x, FFT)
            plan.set_option("register_stages", 1)
        shape = regfft_shape(n, DTYPE[real], on_request=on_request)
        assert shape == kt.shape(r)
        assert plan.describe().startswith(f"stockham registers {shape} one-launch"), (n, real, plan.describe())  # (a silent fall-back shows here)
        for batch in ((7 if r.r3 else 133), 1):
            check(torch, plan, x, truth, batch, REG_L2[real], worst, (n, real, shape))
        if on_request:
            got = guarded(torch, plan, x, FFT)
            assert not np.array_equal(got, want0), (n, real, "another kernel really ran")
            plan.set_option("register_stages", 0)
            assert plan.describe() == base and np.array_equal(guarded(torch, plan, x, FFT), want0), (n, real)
        worst.plans += 1


@pytest.mark.parametrize("real,stages,flag", _reg_cases(), ids=lambda v: str(v))
def test_every_register_stage_row(torch, fa, real, stages, flag):
    """Each adopted (length, precision) of the default rows with this number of stages and variant flag (1 plain, 2 split-plane exchanges,
    3 factored twiddle tables, 4 both, f32 5 / 6 one transform per workgroup without / with factored tables): the plan is the one-launch
    register plan of the row's shape; batches 133 (two stages) / 7 (three) and 1, forward and square-root-scaled inverse, against the f64
    truth within REG_L2 (each transform's largest error within twice that), equal rows of a batch bit-equal, guard bands and input intact."""
    worst = Worst()
    _reg_sweep(torch, fa, real, _reg_rows(real, stages, flag), worst)
    assert worst.plans == len(_reg_rows(real, stages, flag)) > 0
    worst.report(f"register stages {real} {stages} stages flag {flag}: visited {worst.plans} (length, precision) pairs", REG_L2[real])


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_every_register_stage_row_on_request(torch, fa, real):
    """The 2^a 3^b lengths of FOURIER_REGFFT_OPT_ROW in each precision whose flag is not 0: the same checks under plan option
    "register_stages" = 1; by default the plan is the mixed-radix one, another kernel really ran, and 0 restores description and bits."""
    table_rows = [r for r in kt.regfft_rows() if r.on_request and kt.flag(r, real)]
    assert len(table_rows) == kt.regfft_counts()[1][1 if real == "f32" else 2]
    worst = Worst()
    _reg_sweep(torch, fa, real, table_rows, worst, on_request=True)
    worst.report(f"register stages on request {real}: visited {worst.plans} (length, precision) pairs", REG_L2[real])


# ---- (b), (c) every tile-pass length, in every role ----
# tests/golden/table_cover.json (tools/find_table_cover.py, read from describe() of default plans on an MI355X): "plain" rows (n, real, passes):
# per menu length and precision the smallest n whose default plan runs it as FIRST pass and the smallest that runs it as LAST pass, with a
# ragged last tile where a partner of up to 105 points gives one; "blu" rows (n, real, description): per length of the Bluestein menu the
# smallest Bluestein length that takes it as L1 (chirp-in and chirp-out pass) and the smallest that takes it as L2 (conv pass).
COVER = kt.load_cover()
CASE_POINTS = 2_500_000  # a parametrised case holds consecutive rows of the table up to this many points in all

# What no default plan reaches, each with its reason (tools/find_table_cover.py found no plan among all products of two menu lengths and
# all products of three up to 2.5 million points; for the Bluestein roles among all lengths with a prime factor above 13 up to 2^17).
_NO_F64_KERNEL = "f64 has no kernel of this length: a stage of more than 32 points (kernels_regtile.cpp: make_regtile_long)"
_FIRST_TOO_SHORT = ("as the first of two passes L x r it needs r <= L, n <= 10000: such lengths run in one launch (register stages, the LDS "
                    "mixed-radix kernel); and no product of three menu lengths up to 2.5 million points that has no split into two has it as "
                    "its longest pass")
_LAST_SPLITS_EVENLY = ("64 x a and 72 x a run in one launch up to 20480 points; every longer one has a split with a shorter first pass, which "
                       "TiledMixedEngine::factorise prefers (72 x 288 = 144 x 144), and in three passes it is never the shortest")
_LAST_POW2 = "as a last pass it needs 1024 x 1024, a power of two"
_NO_REG_KERNEL = "no register-tile kernel (no split into two stages of at most 32 points; the LDS kernel has no Bluestein roles): not in BluTiledEngine::menu"
_NEVER_CHOSEN = ("BluTiledEngine::choose_m takes it in this role for no Bluestein length whose smooth work array pays (plan.h: init_bluestein; "
                 "restated in tools/find_table_cover.py and applied to every length with a prime factor above 13 up to 2^17)")
PLAIN_UNREACHED = [
    (_FIRST_TOO_SHORT, "f32", "first", [64, 70, 72, 75, 80, 81, 84, 90, 96, 100]),
    (_LAST_SPLITS_EVENLY, "f32", "last", [64, 72]),
    (_LAST_POW2, "f32", "last", [1024]),
    (_FIRST_TOO_SHORT, "f64", "first", [64, 70, 72, 75, 80, 81, 84, 90, 96]),
    (_LAST_SPLITS_EVENLY, "f64", "last", [64, 72]),
    (_LAST_POW2, "f64", "last", [1024]),
    (_NO_F64_KERNEL, "f64", "first", [875, 945, 972, 980, 1000]),
    (_NO_F64_KERNEL, "f64", "last", [875, 945, 972, 980, 1000]),
]
BLU_UNREACHED = [
    (_NO_REG_KERNEL, "f32", "L1", [125, 245, 343, 490]),
    (_NEVER_CHOSEN, "f32", "L1", [64, 70, 72, 75, 80, 81, 84, 90, 96, 98, 100, 105, 108, 112, 120, 126, 128, 135, 140, 144, 147, 150, 160, 162, 168, 175, 180, 189, 192, 216, 224, 225, 243, 250, 350, 375, 384, 392, 448, 512]),
    (_NO_REG_KERNEL, "f32", "L2", [125, 245, 343, 490]),
    (_NEVER_CHOSEN, "f32", "L2", [64, 70, 72, 75, 80, 81, 84, 90, 96, 98, 100, 105, 108, 112, 120, 126, 128, 135, 147, 150, 160, 162, 175, 180, 189, 192, 200, 216, 224, 243, 250, 252, 270, 280, 294, 300, 315, 320, 350, 375, 378, 384, 392, 405, 420, 432, 441, 448, 450, 480, 486, 500, 504, 512]),
    (_NO_REG_KERNEL, "f64", "L1", [125, 245, 343, 490]),
    (_NEVER_CHOSEN, "f64", "L1", [64, 70, 72, 75, 80, 81, 84, 90, 96, 98, 100, 105, 108, 112, 120, 126, 128, 135, 140, 147, 160, 162, 175, 189, 243, 250, 350, 375, 384, 392, 448, 512]),
    (_NO_REG_KERNEL, "f64", "L2", [125, 245, 343, 490]),
    (_NEVER_CHOSEN, "f64", "L2", [64, 70, 72, 75, 80, 81, 84, 90, 98, 105, 126, 128, 135, 147, 150, 160, 162, 175, 180, 189, 192, 200, 216, 224, 243, 250, 252, 270, 280, 294, 300, 315, 320, 350, 375, 378, 384, 392, 405, 420, 432, 441, 448, 450, 480, 486, 500, 504, 512]),
]


def _parts(key, real):
    parts, size = [[]], 0
    for n, r, desc in COVER[key]:
        if r != real:
            continue
        if parts[-1] and size + n > CASE_POINTS:
            parts.append([])
            size = 0
        parts[-1].append((n, desc))
        size += n
    return parts


def _tile_cases(key):
    return [(real, i) for real in ("f32", "f64") for i in range(len(_parts(key, real)))]


def tile_cover_accounts_for_every_length():
    """every menu length, in each precision and role, is in exactly one of the cover table and the reasoned lists above"""
    short, long_ = kt.tile_lengths()
    for key, menu, roles, unreached in (("plain", short + long_, ("first", "last"), PLAIN_UNREACHED), ("blu", short, ("L1", "L2"), BLU_UNREACHED)):
        listed = {}
        for why, real, role, lengths in unreached:
            assert why and lengths == sorted(set(lengths)), (why, real, role)
            for L in lengths:
                assert (L, real, role) not in listed, (L, real, role)
                listed[(L, real, role)] = why
        covered = set()
        for n, real, desc in COVER[key]:
            lens = [int(v) for v in desc.split(" ")[-1].split("x")]
            assert np.prod(lens) == (n if key == "plain" else int(desc.split(" ")[0][2:])), (n, desc)
            covered.add((lens[0], real, roles[0]))
            covered.add((lens[-1], real, roles[1]))
        want = {(L, real, role) for L in menu for real in ("f32", "f64") for role in roles}
        assert covered <= want, sorted(covered - want)
        assert not (covered & set(listed)), sorted(covered & set(listed))
        assert covered | set(listed) == want, (sorted(want - covered - set(listed)), sorted(set(listed) - want))
        assert sorted(map(tuple, COVER[key + "_unreached"])) == sorted(listed), key  # what the tool found no plan for, each with its reason here


def test_tile_cover_accounts_for_every_menu_length():
    tile_cover_accounts_for_every_length()


@pytest.mark.parametrize("real,part", _tile_cases("plain"), ids=lambda v: str(v))
def test_every_tile_pass_length_as_first_and_last_pass(torch, fa, real, part):
    """Each row of the plain cover table: the default plan is "stockham mixed tiles" with exactly the table's passes (a stale table is
    loud); 3 transforms, forward and square-root-scaled inverse, out of place and in place through the guarded runner, against the f64
    truth within TILE_L2.  The lengths 125, 245, 343 and 490 run the LDS kernel of kernels_tiled.cpp (no split into two register stages),
    every other length the register kernel of kernels_regtile.cpp."""
    worst = Worst()
    for n, passes in _parts("plain", real)[part]:
        plan = make(fa, n, real)
        assert plan.describe().startswith(f"stockham mixed tiles {passes} "), (n, real, passes, plan.describe())
        x, truth = inputs_and_truth(n, real, 2)  # (3 transforms: the third repeats the first)
        check(torch, plan, x, truth, 3, TILE_L2[real], worst, (n, real, passes))
        worst.plans += 1
    worst.report(f"tile passes plain {real} part {part}", TILE_L2[real])


@pytest.mark.parametrize("real,part", _tile_cases("blu"), ids=lambda v: str(v))
def test_every_tile_pass_length_in_its_bluestein_roles(torch, fa, real, part):
    """Each row of the Bluestein cover table: the default plan is Bluestein on the table's M = L1 x L2 and launches chirp_in_pass (L1),
    conv_pass (L2), chirp_out_pass (L1); otherwise as the plain rows."""
    worst = Worst()
    for n, desc in _parts("blu", real)[part]:
        plan = make(fa, n, real)
        assert plan.describe().startswith(f"bluestein {desc} "), (n, real, desc, plan.describe())
        x, truth = inputs_and_truth(n, real, 2)
        d = torch.from_numpy(x).cuda()
        o = torch.empty_like(d)
        names = [p[0] for p in plan.profile_batch_ptr(d.data_ptr(), o.data_ptr(), 2, FFT, 0) if p[2] > 0]
        assert names == ["chirp_in_pass", "conv_pass", "chirp_out_pass"], (n, real, names)
        check(torch, plan, x, truth, 3, TILE_L2[real], worst, (n, real, desc))
        worst.plans += 1
    worst.report(f"tile passes bluestein {real} part {part}", TILE_L2[real])
