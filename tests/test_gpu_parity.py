"""Parity tests proper (-m gpu): the HIP engine, called through the C ABI of include/fourier.h,
against the oracle (oracle/fourier_oracle.cpp), the committed golden fixtures, and -- at BASELINE.json's
full sizes -- size-independent properties (round trip, Parseval, linearity) plus sampled transforms.

Tolerances (SURVEY.md section 8c / BASELINE.md section 3):
  small-N sweep: the reference's own 1e-4 | 8 ulp (f32), 1e-11 | 8 ulp (f64)  (integrity.rs:89-143)
  f32 pow2 (N=4096, 2^20, 2^22): rel-L2 <= 1e-6, max <= 2e-6*max|X| ; f64 N=2^20: 5e-14 / 1e-13
  Bluestein f32 N=999983: rel-L2 <= 2e-6, max <= 4e-6*max|X|
"""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, hash_normal, hash_uniform, load_ref10, naive_dft, near, rel_l2, max_rel, regfft_shape, sample_bins

pytestmark = pytest.mark.gpu

F32_EPS, F64_EPS = 1e-4, 1e-11


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
    maps = open("/proc/self/maps").read()
    assert "fourier_amd/lib/libfourier.so" in maps, "the in-tree HIP library must be the one that is loaded"
    return fourier_amd


@pytest.fixture
def fa_exp(torch, fa):
    """The same sources built with -DFOURIER_EXPERIMENTS (fourier_amd/lib/libfourier_experiments.so): the measured-slower
    designs and the environment switches between plans, which the product library does not contain."""
    import ctypes

    from fourier_amd import _lib, build

    if not os.path.exists(build.OUT_EXPERIMENTS):
        pytest.fail("fourier_amd/lib/libfourier_experiments.so is missing: run __graft_entry__.build()")
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    yield fa
    _lib._lib = prev


def make(fa, n, dtype):
    return fa.create_fft_f32(n) if np.dtype(dtype) == np.complex64 else fa.create_fft_f64(n)


def test_product_library_has_no_environment_switches_and_no_experiment_kernels(torch, fa, monkeypatch):
    """Plan selection of libfourier.so does not depend on the environment of the process that links it, and the
    measured-slower designs are not compiled into it."""
    base = {n: make(fa, n, np.complex64).describe() for n in (1 << 14, 1 << 21, 1 << 22, 1 << 23, 96, 999983)}
    for var in ("FOURIER_NO_TWOLEVEL", "FOURIER_WIDE_2048", "FOURIER_SPLIT_2048", "FOURIER_PLAN_4096", "FOURIER_THREE_PASS_2P23",
                "FOURIER_L2_FUSED", "FOURIER_MIX_GENERIC", "FOURIER_MIX_MAX_N", "FOURIER_BLU_SHORT_FIRST", "FOURIER_CONV_XCD_PLAIN",
                "FOURIER_LAUNCH_BYTES", "FOURIER_LAUNCH_ITEMS"):
        monkeypatch.setenv(var, "1")
    assert {n: make(fa, n, np.complex64).describe() for n in base} == base
    with pytest.raises(fa.FourierError):
        make(fa, 1 << 16, np.complex64).set_option("l2_fused", 1)
    with pytest.raises(fa.FourierError):
        make(fa, 1 << 22, np.complex64).set_option("last_pass_prefetch", 1)
    import subprocess

    from fourier_amd import _lib
    syms = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "fft_l2fused_kernel" not in syms and "fft_last_split_kernel" not in syms and "fft_last_prefetch_kernel" not in syms


def gpu_batch(torch, fa, plan, x, code, inplace=False):
    """x: numpy (batch, n) -> device-resident batched transform -> numpy."""
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    o = d if inplace else torch.empty_like(d)
    plan.transform(d, o, fa.Transform(code))
    torch.cuda.synchronize()
    return o.cpu().numpy()


@pytest.mark.parametrize("dtype,eps", [(np.complex64, F32_EPS), (np.complex128, F64_EPS)])
@pytest.mark.parametrize("forward", [True, False])
def test_sweep_1_255_like_reference(fa, oracle, dtype, eps, forward):
    """integrity.rs:145-192 through the legacy host ABI (H2D, transform, D2H inside the library)."""
    g = np.load(os.path.join(GOLDEN, "sweep_1_255.npz"))
    x = (g["x_fwd"] if forward else g["x_inv"]).astype(dtype)
    y64 = g["y_fwd"] if forward else g["y_inv"]
    code = fa.Transform.Fft if forward else fa.Transform.Ifft
    off = 0
    for n in range(1, 256):
        plan = make(fa, n, dtype)
        got = np.empty(n, dtype)
        plan.transform(np.ascontiguousarray(x[:n]), got, code)
        ok, worst = near(naive_dft(x[:n], inverse=not forward), got, eps)
        assert ok, (n, worst)
        want = y64[off:off + n]
        off += n
        scale = max(np.abs(want).max(), 1.0)
        tol = (3e-6 if dtype == np.complex64 else 1e-12) * scale
        assert np.abs(got - want).max() <= tol, (n, float(np.abs(got - want).max()))
        orc = oracle.OracleFft(n, dtype).transform(x[:n], int(code))
        assert np.abs(got - orc).max() <= 2 * tol, n


@pytest.mark.parametrize("dtype,eps", [(np.complex64, F32_EPS), (np.complex128, F64_EPS)])
def test_reference_golden_vector(fa, dtype, eps):
    x, y = load_ref10()
    plan = make(fa, 10, dtype)
    got = np.empty(10, dtype)
    plan.fft(x.astype(dtype), got)
    assert near(got, y, eps)[0]
    plan.ifft(y.astype(dtype), got)
    assert near(got, x, eps)[0]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_ffi_impulse_roundtrip(fa, dtype):
    plan = make(fa, 4, dtype)
    x = np.array([1, 0, 0, 0], dtype=dtype)
    out = np.empty_like(x)
    plan.transform(x, out, fa.Transform.Fft)
    assert np.allclose(out, 1)
    plan.transform_in_place(out, fa.Transform.Ifft)
    assert np.abs(out - x).max() <= 1e-10


@pytest.mark.parametrize("n", [1, 2, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 1 << 14, 1 << 15, 1 << 16, 1 << 18])
@pytest.mark.parametrize("dtype,tl2,tmax", [(np.complex64, 1e-6, 2e-6), (np.complex128, 5e-14, 1e-13)])
def test_pow2_all_codes_vs_oracle(torch, fa, oracle, n, dtype, tl2, tmax):
    plan = make(fa, n, dtype)
    batch = 5 if n <= 4096 else 3
    x = np.stack([hash_normal(900 + b, n) for b in range(batch)]).astype(dtype)
    for code in range(5):
        ref = oracle.transform_batch(x, code)
        for inplace in (False, True):
            got = gpu_batch(torch, fa, plan, x, code, inplace)
            assert rel_l2(got, ref) <= tl2 and max_rel(got, ref) <= tmax, (n, code, inplace, rel_l2(got, ref))


@pytest.mark.parametrize("n", [3, 7, 12, 17, 73, 96, 100, 255, 1000, 1003, 1025, 2500, 4095, 10007, 65537])
def test_bluestein_and_mixed_radix_vs_oracle(torch, fa, oracle, n):
    x = np.stack([hash_normal(40 + b, n) for b in range(3)])
    for dtype, tl2 in ((np.complex64, 2e-6), (np.complex128, 5e-11)):
        plan = make(fa, n, dtype)
        for code in range(5):
            ref = oracle.transform_batch(x.astype(dtype), code)
            assert rel_l2(gpu_batch(torch, fa, plan, x.astype(dtype), code), ref) <= tl2, (n, code)
            assert rel_l2(gpu_batch(torch, fa, plan, x.astype(dtype), code, True), ref) <= tl2, (n, code)
        if dtype == np.complex128:  # against f64 truth the engine is tighter than the oracle's chirp
            assert rel_l2(gpu_batch(torch, fa, plan, x.astype(dtype), 0), np.fft.fft(x, axis=1)) <= 1e-13


def test_config_c1_n4096_spectrum(torch, fa):
    g = np.load(os.path.join(GOLDEN, "n4096.npz"))
    x = hash_normal(int(g["seed"]), 4096)
    for dtype, tl2, tmax in ((np.complex64, 1e-6, 2e-6), (np.complex128, 5e-14, 1e-13)):
        got = gpu_batch(torch, fa, make(fa, 4096, dtype), x.astype(dtype)[None, :], 0)[0]
        assert rel_l2(got, g["y"]) <= tl2 and max_rel(got, g["y"]) <= tmax


@pytest.mark.parametrize("n,dtype,tl2,tmax", [
    (1 << 20, np.complex64, 1e-6, 2e-6),    # C2
    (1 << 20, np.complex128, 5e-14, 1e-13),  # C3
    (999983, np.complex64, 2e-6, 4e-6),     # C4
    (1 << 22, np.complex64, 1e-6, 2e-6),    # C5
])
def test_baseline_sizes_vs_oracle_and_golden(torch, fa, oracle, n, dtype, tl2, tmax):
    g = np.load(os.path.join(GOLDEN, "big_samples.npz"))
    x0 = hash_uniform(int(g[f"seed_{n}"]), n).astype(dtype)
    x = np.stack([x0, hash_uniform(11, n).astype(dtype), hash_uniform(12, n).astype(dtype)])
    plan = make(fa, n, dtype)
    got = gpu_batch(torch, fa, plan, x, 0)
    ref = oracle.transform_batch(x, oracle.FFT, nthreads=3)
    for b in range(3):
        assert rel_l2(got[b], ref[b]) <= tl2 and max_rel(got[b], ref[b]) <= tmax, (n, b, rel_l2(got[b], ref[b]))
    bins = g[f"bins_{n}"]
    assert np.abs(got[0][bins] - g[f"y_{n}"]).max() <= tmax * float(g[f"maxabs_{n}"])
    # inverse, in place, every scaling, on the first transform
    for code in (1, 2, 3, 4):
        gi = gpu_batch(torch, fa, plan, x[:1], code, inplace=True)
        ri = oracle.transform_batch(x[:1], code)
        assert rel_l2(gi, ri) <= tl2, (n, code)


def test_mixed_radix_sizes_are_bit_identical_to_the_oracle(torch, fa, oracle):
    """2^a*3^b <= 18432 (f64: 9216): the reference's radix-4/8/3/2 schedule, tables and operation order on the GPU with
    FMA contraction off -> integer-exact agreement with the CPU restatement (not just a tolerance)."""
    sizes = sorted({(2 ** a) * (3 ** b) for a in range(15) for b in range(1, 10) if (2 ** a) * (3 ** b) <= 18432}) + [19683]  # 3^9: 154 KiB of LDS
    for n in sizes:
        x = np.stack([hash_normal(11 + b, n) for b in range(4)])
        for dtype in (np.complex64, np.complex128):
            if n > (19683 if dtype == np.complex64 else 9216) or n == 12288:  # one LDS buffer must fit a workgroup;
                continue                                                       # 3*2^12 takes the tiled passes + odd pass
            plan = make(fa, n, dtype)
            assert "mixed-radix" in plan.describe()
            for code in range(5):
                ref = oracle.transform_batch(x.astype(dtype), code)
                assert np.array_equal(gpu_batch(torch, fa, plan, x.astype(dtype), code), ref), (n, dtype, code)
            assert np.array_equal(gpu_batch(torch, fa, plan, x.astype(dtype), 0, inplace=True),
                                  oracle.transform_batch(x.astype(dtype), 0)), n


@pytest.mark.parametrize("n", [3 * 4096, 9 * 4096, 27 * 4096, 3 * (1 << 15), 9 * (1 << 16), 3 * (1 << 18), 27 * (1 << 16), 3 * (1 << 23),
                               81 * 4096, 243 * 4096, 729 * (1 << 13), 2187 * 4096, 81 * (1 << 17)])
def test_large_mixed_radix_sizes_vs_oracle(torch, fa, oracle, n):
    """2^a*3^b (a >= 12, any b) natively: big-radix passes over 2^a, then radix-27/9/3 passes (middle ones twiddled) -- or two
    mixed-length tile passes where the length splits into two tile lengths of at most 576 (round 6: register tiles, lengths beyond 512 points on
    64-byte rows; round 4: 384)."""
    x = np.stack([hash_uniform(90 + b, n) for b in range(2)])
    for dtype, tl2 in ((np.complex64, 1e-6), (np.complex128, 5e-14)):
        if n > (1 << 24) and dtype == np.complex128:
            continue
        plan = make(fa, n, dtype)
        d = plan.describe()
        assert d.startswith("stockham") and ("mixed tiles" in d or "x3" in d.replace("x9", "x3").replace("x27", "x3")), d
        assert ("mixed tiles" in d) == (n in (3 * 4096, 9 * 4096, 27 * 4096, 3 * (1 << 15), 81 * 4096)), d  # 128x96, 192x192, 384x288, 384x256, 576x576
        for code in (0, 1, 3):
            ref = oracle.transform_batch(x.astype(dtype), code, nthreads=2)
            assert rel_l2(gpu_batch(torch, fa, plan, x.astype(dtype), code), ref) <= tl2, (n, code)
        assert rel_l2(gpu_batch(torch, fa, plan, x.astype(dtype), 0, inplace=True),
                      oracle.transform_batch(x.astype(dtype), 0, nthreads=2)) <= tl2


def test_bluestein_fusion_matches_unfused(torch, fa):
    for n in (17, 127, 439, 1025, 3127, 10007, 999983):  # one-launch chirp-z (M <= 2^15) and pass-fused (M = 2^21)
        x = np.stack([hash_uniform(70 + b, n) for b in range(2)]).astype(np.complex64)
        fused, plain = make(fa, n, np.complex64), make(fa, n, np.complex64)
        plain.set_option("bluestein_fusion", 0)
        for code in (0, 1, 4):
            a, b = gpu_batch(torch, fa, fused, x, code), gpu_batch(torch, fa, plain, x, code)
            assert rel_l2(a, b) <= 4e-7, (n, code, rel_l2(a, b))  # different factorisation order, same tolerance class
            assert np.array_equal(gpu_batch(torch, fa, fused, x, code, inplace=True), a), (n, code)


@pytest.mark.parametrize("n,dtype,tol", [(20002, np.complex64, 2e-6), (40001, np.complex64, 2e-6), (65537, np.complex64, 2e-6),
                                         (999983, np.complex64, 2e-6), (2200000, np.complex64, 2e-6),
                                         (10001, np.complex128, 5e-11), (70001, np.complex128, 5e-11),
                                         (999983, np.complex128, 1e-9)])
def test_bluestein_conv_kernel_vs_separate_passes_and_oracle(torch, fa, oracle, n, dtype, tol):
    """Large Bluestein: last forward pass + (.) w + first inverse pass in one launch (conv_pass) against the
    separate-pass form and the oracle, every transform code, in and out of place."""
    x = np.stack([hash_uniform(170 + b, n) for b in range(2)]).astype(dtype)
    conv, plain = make(fa, n, dtype), make(fa, n, dtype)
    for p in (conv, plain):
        p.set_option("bluestein_smooth_m", 0)  # the power-of-two work array (65537 f32, 10001 f64 take a smooth M by default: round 6)
    plain.set_option("bluestein_conv", 0)
    d = torch.from_numpy(x).cuda()
    o = torch.empty_like(d)
    names = [p[0] for p in conv.profile_batch_ptr(d.data_ptr(), o.data_ptr(), 2, 0, 0) if p[2] > 0]
    assert "conv_pass" in names and "inv_pass0" not in names, names
    for code in range(5):
        a, b = gpu_batch(torch, fa, conv, x, code), gpu_batch(torch, fa, plain, x, code)
        assert rel_l2(a, b) <= (3e-7 if dtype == np.complex64 else 1e-15), (n, code, rel_l2(a, b))
        assert np.array_equal(gpu_batch(torch, fa, conv, x, code, inplace=True), a), (n, code)
        if code in (0, 1):
            ref = oracle.transform_batch(x, code, nthreads=2)
            assert rel_l2(a, ref) <= tol, (n, code, rel_l2(a, ref))


def test_bluestein_reference_chirp_reproduces_the_reference_to_f64_rounding(torch, fa, oracle):
    """Where this engine and the reference differ in f64 Bluestein, the difference is the REFERENCE's: it evaluates the chirp angle
    k^2 * pi / N unreduced in f64 (bluesteins.rs:10,31,57), which costs N * 1e-16 of angle -- 1.7e-10 of the result at N = 999983 --,
    the engine reduces k^2 mod 2N exactly first.  Plan option "bluestein_reference_chirp" builds the tables from the reference's own
    expression: the engine then agrees with the CPU restatement to f64 ROUNDING (1e-15 class) on every Bluestein route -- the one-launch
    kernels, the fused passes with the conv kernel, C4's length --, forward and inverse, while by default it agrees with the exact DFT
    to 1e-15 and with the oracle only as well as the oracle does (which is what the 1e-9 tolerances elsewhere in this file allow for)."""
    for n in (1013, 10007, 65537, 250007, 999983):
        x = np.stack([hash_normal(900 + b, n) for b in range(2)]).astype(np.complex128)
        truth = torch.fft.fft(torch.from_numpy(x)).numpy()
        ref = oracle.transform_batch(x, 0, nthreads=2)
        oracle_err = rel_l2(ref, truth)
        plan = make(fa, n, np.complex128)
        assert "bluestein" in plan.describe()
        got = gpu_batch(torch, fa, plan, x, 0)
        assert rel_l2(got, truth) <= 5e-15, (n, rel_l2(got, truth))              # the engine: the exact DFT
        assert rel_l2(got, ref) <= 1.5 * oracle_err + 1e-14, (n, rel_l2(got, ref))  # ... as far from the oracle as the oracle is from it
        plan.set_option("bluestein_reference_chirp", 1)
        for code in (0, 1, 4):
            r = oracle.transform_batch(x, code, nthreads=2)
            g = gpu_batch(torch, fa, plan, x, code)
            assert rel_l2(g, r) <= 5e-15, (n, code, rel_l2(g, r))               # the reference's results, to rounding
            assert np.array_equal(gpu_batch(torch, fa, plan, x, code, inplace=True), g), (n, code)
        assert abs(rel_l2(gpu_batch(torch, fa, plan, x, 0), truth) - oracle_err) <= 0.2 * oracle_err + 1e-14  # ... and its error
        plan.set_option("bluestein_reference_chirp", 0)
        assert np.array_equal(gpu_batch(torch, fa, plan, x, 0), got), n          # back to the default tables, bit for bit
    with pytest.raises(fa.FourierError):
        make(fa, 4096, np.complex128).set_option("bluestein_reference_chirp", 1)  # not a Bluestein plan
    # f32: the angle error is far below f32 resolution; the option changes nothing measurable
    x = np.stack([hash_normal(910 + b, 10007) for b in range(2)]).astype(np.complex64)
    plan = make(fa, 10007, np.complex64)
    a = gpu_batch(torch, fa, plan, x, 0)
    plan.set_option("bluestein_reference_chirp", 1)
    assert rel_l2(gpu_batch(torch, fa, plan, x, 0), a) <= 2e-7


def test_random_sizes_batches_codes_vs_oracle(torch, fa, oracle):
    """Seeded random sweep over every plan family: random size (1..70000), batch, transform code, precision,
    in/out of place, against the CPU restatement of the reference."""
    rng = np.random.default_rng(20260926)
    sizes = [int(v) for v in rng.integers(1, 6000, 150)] + [int(v) for v in rng.integers(6000, 70000, 40)]
    for n in sizes:
        dtype = np.complex64 if rng.integers(0, 2) else np.complex128
        batch = int(rng.integers(1, 9))
        code = int(rng.integers(0, 5))
        x = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(dtype)
        plan = make(fa, n, dtype)
        ref = oracle.transform_batch(x, code)
        tol = 2e-6 if dtype == np.complex64 else 5e-11
        for inplace in (False, True):
            got = gpu_batch(torch, fa, plan, x, code, inplace)
            assert rel_l2(got, ref) <= tol, (n, plan.describe(), batch, code, inplace, rel_l2(got, ref))


def test_three_pass_size(torch, fa_exp, monkeypatch):
    """2^23 both ways: the default two-pass plan 4096 x 2048 and the three-pass plan 256 x 256 x 128
    (FOURIER_THREE_PASS_2P23=1, experiments build), f32 and f64."""
    fa = fa_exp
    n = 1 << 23
    rng = np.random.default_rng(7)
    for dtype, tol in ((np.complex64, 1e-6), (np.complex128, 5e-14)):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)[None, :]
        ref = np.fft.fft(x[0].astype(np.complex128))
        monkeypatch.setenv("FOURIER_THREE_PASS_2P23", "1")
        three = make(fa, n, dtype)
        monkeypatch.delenv("FOURIER_THREE_PASS_2P23")
        monkeypatch.setenv("FOURIER_TWO_PASS_2P23", "1")  # f64: the two-pass plan is opt-in (no consistent gain)
        two = make(fa, n, dtype)
        monkeypatch.delenv("FOURIER_TWO_PASS_2P23")
        assert "256x256x128" in three.describe() and "4096x2048" in two.describe()
        assert ("4096x2048" if dtype == np.complex64 else "256x256x128") in make(fa, n, dtype).describe()
        for plan in (three, two):
            assert rel_l2(gpu_batch(torch, fa, plan, x, 0)[0], ref) <= tol
            assert rel_l2(gpu_batch(torch, fa, plan, x, 0, inplace=True)[0], ref) <= tol


def _full_size_properties(torch, fa, oracle, n, batch, dtype, tl2, chunk_bytes=None):
    """BASELINE full sizes: round trip, Parseval, linearity, plus sampled transforms vs the oracle."""
    cdt = torch.complex64 if dtype == np.complex64 else torch.complex128
    plan = make(fa, n, dtype)
    if chunk_bytes is not None:
        plan.set_option("chunk_bytes", chunk_bytes)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.empty((batch, n), dtype=cdt, device="cuda")
    torch.view_as_real(x).normal_(0.0, 1.0, generator=gen)
    y = torch.empty_like(x)
    plan.transform(x, y, fa.Transform.Fft)
    torch.cuda.synchronize()
    # sampled transforms vs the oracle (first, middle, last -> batch indexing / chunking)
    idx = [0, batch // 2, batch - 1]
    hx = np.stack([x[i].cpu().numpy() for i in idx])
    ref = oracle.transform_batch(hx, oracle.FFT, nthreads=3)
    for k, i in enumerate(idx):
        assert rel_l2(y[i].cpu().numpy(), ref[k]) <= tl2, (n, i)
    # Parseval on every transform: sum|Y|^2 = N * sum|X|^2
    ex = torch.view_as_real(x).double().pow(2).sum(dim=(1, 2)) if batch * n <= (1 << 28) else None
    if ex is None:
        worst = 0.0
        for b0 in range(0, batch, 256):
            ex_ = torch.view_as_real(x[b0:b0 + 256]).double().pow(2).sum(dim=(1, 2))
            ey_ = torch.view_as_real(y[b0:b0 + 256]).double().pow(2).sum(dim=(1, 2))
            worst = max(worst, float(((ey_ / n - ex_).abs() / ex_).max()))
    else:
        ey = torch.view_as_real(y).double().pow(2).sum(dim=(1, 2))
        worst = float(((ey / n - ex).abs() / ex).max())
    assert worst <= 10 * tl2, worst
    # round trip in place: Ifft(Fft(x)) == x on the whole batch
    plan.transform_in_place(y, fa.Transform.Ifft)
    torch.cuda.synchronize()
    worst = 0.0
    for b0 in range(0, batch, 256):
        d = torch.view_as_real(y[b0:b0 + 256] - x[b0:b0 + 256]).double().pow(2).sum(dim=(1, 2)).sqrt()
        r = torch.view_as_real(x[b0:b0 + 256]).double().pow(2).sum(dim=(1, 2)).sqrt()
        worst = max(worst, float((d / r).max()))
    assert worst <= 2 * tl2, worst
    del x, y
    torch.cuda.empty_cache()


def test_full_size_c2_f32_2p20_batch4096(torch, fa, oracle):
    _full_size_properties(torch, fa, oracle, 1 << 20, 4096, np.complex64, 1e-6)


def test_full_size_c2_chunked(torch, fa, oracle):
    _full_size_properties(torch, fa, oracle, 1 << 20, 512, np.complex64, 1e-6, chunk_bytes=64 << 20)


def test_full_size_c3_f64_2p20_batch4096(torch, fa, oracle):
    _full_size_properties(torch, fa, oracle, 1 << 20, 4096, np.complex128, 5e-14)


def test_full_size_c4_bluestein_batch512(torch, fa, oracle):
    _full_size_properties(torch, fa, oracle, 999983, 512, np.complex64, 2e-6)


def test_c5_chunk_of_2p22(torch, fa, oracle):
    # C5 is 65536 transforms = 2 TiB: executed as fixed chunks; one 256-transform chunk here
    _full_size_properties(torch, fa, oracle, 1 << 22, 256, np.complex64, 1e-6)


@pytest.mark.parametrize("dtype,ks,tl2", [(np.complex64, (16, 17, 18), 1e-6), (np.complex128, (15, 16, 17), 5e-14)])
def test_xcd_fused_one_launch_plan_equals_the_two_launch_plan(torch, fa_exp, oracle, dtype, ks, tl2):
    """Plan option l2_fused: both passes in ONE launch, the intermediate parked in the XCD's L2 (persistent workgroups,
    per-XCD work queues keyed by the hardware XCC id, data-flow waits).  Same arithmetic as the two-launch plan, so the
    results must be bit-identical to it -- for a batch large enough that every XCD queue wraps its window ring many
    times, a ragged batch of 1, in place, and all five transform codes -- and match the oracle.  (Experiments build.)"""
    fa = fa_exp
    for k in ks:
        n = 1 << k
        batch = max(3, (1 << 28) // (n * np.dtype(dtype).itemsize))  # 256 MiB: thousands of queue items per XCD
        two, one = make(fa, n, dtype), make(fa, n, dtype)
        one.set_option("l2_fused", 1)
        assert "xcd-l2" in one.describe() and "xcd-l2" not in two.describe()
        cdt = torch.complex64 if dtype == np.complex64 else torch.complex128
        g = torch.Generator(device="cuda")
        g.manual_seed(1234 + k)
        x = torch.empty((batch, n), dtype=cdt, device="cuda")
        torch.view_as_real(x).normal_(0.0, 1.0, generator=g)
        for code in range(5):
            a, b = torch.empty_like(x), torch.full_like(x, float("nan"))
            two.transform(x, a, fa.Transform(code))
            one.transform(x, b, fa.Transform(code))
            torch.cuda.synchronize()
            assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), (k, code)
        z = x.clone()
        one.transform(z, z, fa.Transform.Fft)   # in place: a transform is read completely before any of it is written
        two.transform(x, a, fa.Transform.Fft)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(z)), k
        for nb in (1, 2, 9):  # fewer transforms than XCDs / than workgroups
            one.transform(x[:nb], b[:nb], fa.Transform.Fft)
            torch.cuda.synchronize()
            assert torch.equal(torch.view_as_real(a[:nb]), torch.view_as_real(b[:nb])), (k, nb)
        ref = oracle.transform_batch(x[:2].cpu().numpy(), oracle.FFT)
        assert rel_l2(b[:2].cpu().numpy(), ref) <= tl2, k
        # the inter-workgroup hand-offs under UNEVEN load: a second stream keeps part of the chip busy with copies
        # while the fused plan runs (workgroups then progress at different speeds); every word must still match
        side = torch.cuda.Stream()
        noise_src = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
        noise_dst = torch.empty_like(noise_src)
        two.transform(x, a, fa.Transform.Fft)
        torch.cuda.synchronize()
        for rep in range(3):
            b.fill_(float("nan"))
            with torch.cuda.stream(side):
                for _ in range(4):
                    noise_dst[rep::7].copy_(noise_src[rep::7], non_blocking=True)  # strided: many small, slow workgroups
            one.transform(x, b, fa.Transform.Fft)
            torch.cuda.synchronize()
            assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), (k, "under load", rep)
        del noise_src, noise_dst
        with pytest.raises(fa.FourierError):
            make(fa, 1 << 20, dtype).set_option("l2_fused", 1)  # the intermediate must fit the XCD's L2
        del x, a, b, z
        torch.cuda.empty_cache()


def test_l2048_passes_narrow_first_and_split_last_match_the_wide_kernels(torch, fa_exp, oracle, monkeypatch):
    """2^21 / 2^22 / Bluestein M = 2^21.  Default plans run the L = 2048 FIRST pass on 64-byte-wide tiles (same
    arithmetic as the 16-column kernel, FOURIER_WIDE_2048=1: bit-identical).  The half-tile LAST pass (two workgroups
    per column tile, radix-2 decimation in frequency in front of a 1024-point tile; FOURIER_SPLIT_2048=1, measured
    slower and therefore off by default) adds one twiddle rounding.  All three against each other and the oracle,
    in and out of place.  (Experiments build: the product library has neither the switches nor the half-tile kernel.)"""
    fa = fa_exp
    for n, batch, tol in ((1 << 21, 5, 1e-6), (1 << 22, 3, 1e-6), (999983, 2, 2e-6)):
        x = np.stack([hash_normal(50 + b, n) for b in range(batch)]).astype(np.complex64)
        new = make(fa, n, np.complex64)
        monkeypatch.setenv("FOURIER_WIDE_2048", "1")
        old = make(fa, n, np.complex64)
        monkeypatch.delenv("FOURIER_WIDE_2048")
        monkeypatch.setenv("FOURIER_SPLIT_2048", "1")
        split = make(fa, n, np.complex64)
        monkeypatch.delenv("FOURIER_SPLIT_2048")
        ref = oracle.transform_batch(x[:1], oracle.FFT)
        for inplace in (False, True):
            yn = gpu_batch(torch, fa, new, x, 0, inplace=inplace)
            yo = gpu_batch(torch, fa, old, x, 0, inplace=inplace)
            ys = gpu_batch(torch, fa, split, x, 0, inplace=inplace)
            assert np.array_equal(yn, yo), (n, inplace)
            assert rel_l2(ys, yo) <= 3e-7, (n, inplace, rel_l2(ys, yo))
            assert rel_l2(yn[0], ref[0]) <= tol and rel_l2(ys[0], ref[0]) <= tol, (n, inplace)
        back = gpu_batch(torch, fa, new, yn, 1)
        assert rel_l2(back, x) <= 2 * tol, n


def test_c5_full_job_65536_transforms_on_one_gpu(torch, fa, oracle):
    """BASELINE configs[4] as specified, on ONE GPU: f32 N=2^22, batch 65536 = 2 TiB of input, walked as 64 resident
    chunks of 1024 transforms (32 GiB), every chunk regenerated on the device (seed = global chunk index) and
    transformed out of place -- the loop `bench.py --config c5` times.  Checked: Parseval on EVERY chunk (energy of
    all 1024 transforms; a chunk that was skipped, or transformed with the wrong stride, fails it), and 66 transforms
    against the oracle: one per chunk plus the first and the last of the job."""
    n, gbatch, chunk = 1 << 22, 65536, 1024
    plan = fa.create_fft_f32(n)
    x = torch.empty((chunk, n), dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    gen = torch.Generator(device="cuda")
    orc = oracle.OracleFft(n, np.complex64)
    checked = 0
    for c, b0 in enumerate(range(0, gbatch, chunk)):
        gen.manual_seed(0xC5000 + b0)
        torch.view_as_real(x).uniform_(-1.0, 1.0, generator=gen)
        plan.transform(x, y, fa.Transform.Fft)
        ex = torch.view_as_real(x).double().pow(2).sum(dim=(1, 2))
        ey = torch.view_as_real(y).double().pow(2).sum(dim=(1, 2)) / n
        assert float(((ey - ex).abs() / ex).max()) < 2e-6, (c, "Parseval")
        # against the oracle: one transform of EVERY chunk, at a row that moves through the chunk from chunk to chunk (every
        # residue of the 1024 rows modulo 64 and both halves of the chunk are visited), plus the job's first and last transform
        rows = {(c * 611 + 17) % chunk} | ({0} if c == 0 else set()) | ({chunk - 1} if b0 + chunk == gbatch else set())
        for row in sorted(rows):
            ref = orc.transform(x[row].cpu().numpy(), oracle.FFT)
            assert rel_l2(y[row].cpu().numpy(), ref) <= 1e-6, (c, row)
            checked += 1
    assert checked == gbatch // chunk + 2
    del x, y
    torch.cuda.empty_cache()


def test_two_devices_driven_from_two_host_threads_in_one_process(torch, fa, oracle):
    """one host thread + one HIP stream per device, batch split contiguously, through
    fourier_hip_create_*(size, device).  Needs two GPUs in this process (skipped on a one-GPU box; the same driver
    object is exercised with two shards on ONE device below so the code path itself always runs)."""
    from fourier_amd import shard

    n, gbatch = 1 << 16, 64
    ndev = torch.cuda.device_count()
    devices = [0, 1] if ndev >= 2 else [0, 0]
    x = hash_normal(77, gbatch * n).astype(np.complex64).reshape(gbatch, n)
    ref = oracle.transform_batch(x, oracle.FFT)
    drv = shard.DeviceShardedFft(n, "f32", devices)
    ins, outs = [], []
    for g, d in enumerate(devices):
        lo, hi = shard.batch_shard(gbatch, len(devices), g)
        ins.append(torch.from_numpy(x[lo:hi]).to(f"cuda:{d}"))
        outs.append(torch.empty_like(ins[-1]))
    drv.transform(ins, outs, fa.Transform.Fft)
    got = np.concatenate([o.cpu().numpy() for o in outs])
    assert rel_l2(got, ref) <= 1e-6
    assert [p.device for p in drv.plans] == devices
    if ndev >= 2:
        with pytest.raises(ValueError):  # a tensor on the wrong device is rejected, not launched
            drv.transform([ins[1], ins[0]], outs, fa.Transform.Fft)
    else:
        pytest.skip("one GPU visible: ran both shards on cuda:0 (two plans, two threads, two streams)")


def test_sharded_driver_orders_against_the_callers_stream_and_returns_when_done(torch, fa):
    """DeviceShardedFft (round-2 advisor): (1) inputs produced on the CALLER's non-default stream are waited for -- the
    worker threads look up nothing thread-local; (2) the raw (pointer, batch) form has finished when transform() returns
    (it synchronises through fourier_hip_synchronize_*): a copy on an unrelated non-blocking stream right after must see
    complete results.  Large enough that an unordered launch would run ahead of the producer / the copy."""
    from fourier_amd import shard

    n, per = 1 << 20, 96  # 2 x 768 MiB per shard: tens of milliseconds of kernels
    drv = shard.DeviceShardedFft(n, "f32", [0, 0])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ins = []
        for g in range(2):
            x = torch.zeros((per, n), dtype=torch.complex64, device="cuda")
            for _ in range(4):
                x.add_(0.25)  # the producer is still running on `side` when transform() is called
            ins.append(x)
        outs = [torch.full_like(x, float("nan")) for x in ins]
        drv.transform(ins, outs, fa.Transform.Fft)  # current stream of THIS thread = side
    for o in outs:  # a constant input: X[0] = n, everything else 0
        assert torch.allclose(o[:, 0].real, torch.full((per,), float(n), device="cuda")) and float(o[:, 1:].abs().max()) < 1e-2
    torch.cuda.synchronize()
    raw_out = [torch.full_like(x, float("nan")) for x in ins]
    drv.transform([(x.data_ptr(), per) for x in ins], [(o.data_ptr(), per) for o in raw_out], fa.Transform.Fft)
    other = torch.cuda.Stream()  # non-blocking: no implicit ordering with the NULL stream the raw form runs on
    with torch.cuda.stream(other):
        copies = [o.clone() for o in raw_out]
    other.synchronize()
    for c, o in zip(copies, outs):
        assert torch.equal(torch.view_as_real(c), torch.view_as_real(o))


def test_bench_strong_scaling_path_with_two_ranks(torch, fa, tmp_path):
    """`bench.py --gpus 2 --full` as the driver launches it (torch.distributed.run, one rank per GPU): BASELINE
    configs[4] with the global batch split over the ranks, "scaling": "strong", one JSON line from rank 0, with the
    parity, roofline and single-GPU reference legs of --full.  With two GPUs it runs over RCCL; on a one-GPU box the two
    ranks share cuda:0 (BENCH_SHARE_DEVICES) and, because RCCL refuses two ranks on one device, the group is gloo -- the
    data path has no collective either way.  A reduced global batch keeps it short; the plan, chunking, sharding and JSON
    contract are the full-size ones."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    two = torch.cuda.device_count() >= 2
    if not two:
        env.update(BENCH_SHARE_DEVICES="1", BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1536", "--chunk", "256", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # exactly one JSON line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["steps"] == 2
    assert out["config"]["global_batch"] == 1536 and out["config"]["batch_per_gpu"] == 768 and out["config"]["n"] == 1 << 22
    assert "BASELINE configs[4]" in out["config"]["workload"]
    assert out["parity"]["rel_l2_vs_oracle"] <= 1e-6
    assert out["value"] > 0 and out["roofline"]["frac"] > 0.3
    # value = whole job: global batch * 5 N log2 N / max-over-ranks FFT time
    assert abs(out["value"] - 1536 * 5 * (1 << 22) * 22 / (out["ms_per_step"] * 1e-3) / 1e9) / out["value"] < 1e-3
    # the line judges its own scaling: configuration key, process group, every rank's time, an in-run one-GPU reference
    assert out["config_key"] == "c5" and out["process_group"]["world_size"] == 2
    assert out["process_group"]["backend"] == ("nccl" if two else "gloo")
    ss = out["strong_scaling"]
    assert len(ss["per_rank_fft_ms_per_step"]) == 2 and ss["transforms_per_rank"] == [768, 768]
    assert sum(ss["transforms_per_rank"]) == out["config"]["global_batch"] and "efficiency_vs_reference" in ss
    assert abs(max(ss["per_rank_fft_ms_per_step"]) - out["ms_per_step"]) / out["ms_per_step"] < 1e-3  # ms_per_step = slowest rank
    assert ss["single_gpu_reference"]["chunk"] == 256 and ss["single_gpu_reference"]["ms_per_chunk"] > 0
    assert abs(ss["ideal_ms_per_step"] - ss["single_gpu_reference"]["ms_per_chunk"] * 3) < 1e-2  # 768 per rank = 3 chunks
    assert 0 < ss["efficiency_vs_reference"] <= (1.25 if two else 1.05)  # two ranks on ONE shared GPU: about 0.5


@pytest.mark.parametrize("config", ["c2", "c5"])
def test_bench_dump_outputs_is_the_last_timed_step(torch, fa, oracle, tmp_path, config):
    """`bench.py --dump-outputs DIR` writes a fixed sample of what its last timed step computed: the same files bit for bit
    from two runs with the same arguments, at most 64 MB, and equal to the output of this process's own plan on the inputs
    bench.py generates (c2: one resident batch; c5: every chunk of the last step, regenerated from its seed)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, batch, chunk, steps = 1 << 16, 1024, 256, 3  # 512 MiB of output: more than the dump takes, so it is sampled
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
               "--config", config, "--log2n", "16", "--batch", str(batch), "--chunk", str(chunk), "--no-cpu", "--no-other",
               "--no-ceiling", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == steps
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == ["output_points.npy", "output_rows.npy"] == sorted(p.name for p in dirs[1].iterdir())
    assert sum(p.stat().st_size for p in dirs[0].iterdir()) <= 64 * 10**6
    got = {k: np.load(dirs[0] / f"output_{k}.npy") for k in ("rows", "points")}
    for k in got:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], np.load(dirs[1] / f"output_{k}.npy"))
    assert got["rows"].shape[1:] == (n, 2) and got["points"].shape[1:] == (2,)

    # the same transforms in this process: bench.py's inputs, the same plan
    plan = fa.create_fft_f32(n, 0)
    x = torch.empty((batch, n), dtype=torch.complex64, device="cuda")
    if config == "c2":
        torch.manual_seed(0x5EED0001)
        torch.view_as_real(x).uniform_(0.0, 1.0)
    else:
        gen = torch.Generator(device="cuda")
        for b0 in range(0, batch, chunk):
            gen.manual_seed(0x5EED0C50 + 7919 * (steps - 1) + b0)
            torch.view_as_real(x[b0:b0 + chunk]).uniform_(0.0, 1.0, generator=gen)
    y = torch.empty_like(x)
    plan.transform(x, y, fa.Transform.Fft)
    torch.cuda.synchronize()
    yr = torch.view_as_real(y).cpu().numpy()
    sys.path.insert(0, root)
    import bench

    sample = bench.OutputSample(batch, n, 8, bench.DUMP_BYTES)  # the seeded sample is a function of the shape alone
    assert sample.rows[0] == 0 and sample.rows[-1] == batch - 1 and len(sample.points) > 0
    assert np.array_equal(got["rows"], yr[sample.rows])
    assert np.array_equal(got["points"], yr.reshape(-1, 2)[sample.points])
    ref = oracle.transform_batch(x[-1:].cpu().numpy(), oracle.FFT)  # and the last transform is right
    assert rel_l2(got["rows"][-1].view(np.complex64).ravel(), ref[0]) <= 1e-6


def test_bench_plain_run_is_the_headline_alone_and_full_adds_the_legs(torch, fa, tmp_path):
    """A plain `bench.py` run prints the headline line without the legs that take runs of their own (roofline, parity /
    cpu_baseline, other_configs, the c5 single-GPU reference); `--full` adds them to the same line."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    legs = {"roofline", "parity", "cpu_baseline", "other_configs"}

    def run(*extra):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2n", "16", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        return json.loads(lines[0])

    for config, extra in (("c2", ["--batch", "2048"]), ("c5", ["--batch", "2048", "--chunk", "1024"])):
        out = run("--config", config, *extra)
        assert not legs & set(out), sorted(legs & set(out))
        assert out["config_key"] == config and out["steps"] == 2 and out["warmup"] == 1
        assert out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and "N=2^16" in out["metric"]
        assert abs(out["value"] - 2048 * 5 * (1 << 16) * 16 / (out["ms_per_step"] * 1e-3) / 1e9) / out["value"] < 1e-2
        if config == "c5":
            assert out["strong_scaling"]["transforms_per_rank"] == [2048] and "single_gpu_reference" not in out["strong_scaling"]

    out = run("--config", "c2", "--batch", "2048", "--full", "--cpu-sample", "4")
    assert {"roofline", "parity", "cpu_baseline"} <= set(out)
    assert out["parity"]["rel_l2_vs_oracle"] <= 1e-6 and out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0


def test_device_and_overlap_checks_of_the_operator_layer(torch, fa):
    plan = fa.create_fft_f32(256, 0)
    assert plan.device == 0
    x = torch.zeros(4 * 256, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):  # partial overlap (include/fourier.h forbids it)
        plan.transform(x[:512], x[256:768], fa.Transform.Fft)
    plan.transform(x[:512], x[512:], fa.Transform.Fft)  # disjoint halves of one allocation are fine
    plan.transform(x[:512], x[:512], fa.Transform.Fft)  # same buffer = in place
    torch.cuda.synchronize()


def test_reserve_then_capture_without_warmup(torch, fa, oracle):
    """fourier_hip_reserve_*: after reserve(batch, in_place) the very first in-place call allocates nothing, so it can
    be captured into a HIP graph without a warm-up call."""
    n, batch = 1 << 16, 8
    x = hash_normal(5, batch * n).astype(np.complex64).reshape(batch, n)
    d = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    other = fa.create_fft_f32(n)  # loads the kernels' code object (first launch of a module is not capturable)
    with torch.cuda.stream(side):
        other.transform(d.clone(), d.clone(), fa.Transform.Fft)
    side.synchronize()
    plan = fa.create_fft_f32(n)
    plan.reserve(batch, in_place=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        plan.transform(d, d, fa.Transform.Fft)  # FIRST call on this plan: captured, must not allocate
    g.replay()
    torch.cuda.synchronize()
    assert rel_l2(d.cpu().numpy(), oracle.transform_batch(x, oracle.FFT)) <= 1e-6


def test_stream_pipeline_option_on_the_gpu(torch, fa, oracle):
    """Plan option "stream_pipeline" (round 6): pass 0 of chunk k+1 on one internal stream beside pass 1 of chunk k on another,
    ordered by events only, intermediate in a plan-owned ring.  Real concurrency here (the emulator runs it serially): the same
    bits as the two whole-batch launches, out of place and in place, repeated calls reusing ring and events, ragged last chunk,
    inside the caller's stream order (the input is produced and the output consumed on the caller's stream without a sync)."""
    for n, batch, dtype in ((1 << 20, 37, np.complex64), (1 << 16, 203, np.complex64), (1 << 18, 21, np.complex128)):
        cdt = torch.complex64 if dtype == np.complex64 else torch.complex128
        x = torch.from_numpy(hash_normal(61, batch * n).astype(dtype).reshape(batch, n)).cuda()
        base = torch.empty_like(x)
        make(fa, n, dtype).transform(x, base, fa.Transform.Fft)
        torch.cuda.synchronize()
        for chunk, slots, one in ((1, 2, 0), (4, 3, 0), (8, 2, 0), (5, 4, 1), (64, 2, 0)):
            plan = make(fa, n, dtype)
            plan.set_option("stream_pipeline", chunk | slots << 16 | one << 24)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(3):
                    xs = x * 1.0        # produced on the caller's stream right before the call
                    y = torch.zeros_like(x)
                    plan.transform(xs, y, fa.Transform.Fft)
                    ok = torch.equal(torch.view_as_real(y), torch.view_as_real(base))  # consumed on the caller's stream right after it
                    assert ok, (n, chunk, slots, one)
                plan.transform_in_place(xs, fa.Transform.Fft)
                assert torch.equal(torch.view_as_real(xs), torch.view_as_real(base)), (n, chunk, slots, "in place")
            side.synchronize()
        del x, base
        torch.cuda.empty_cache()


@pytest.mark.parametrize("log2n,dtype,tol", [(27, np.complex64, 1e-6), (26, np.complex128, 5e-14), (30, np.complex64, 1.5e-6)])
def test_largest_three_pass_sizes_known_answers(torch, fa, log2n, dtype, tol):
    """2^26 .. 2^30 (three passes, 1..8 GiB per transform): too long for the CPU oracle, so pinned by known answers
    computed on the device in f64 -- a shifted impulse plus a tone transforms to a pure phase ramp plus a single
    bin -- and by the in-place round trip."""
    n = 1 << log2n
    cdt = torch.complex64 if dtype == np.complex64 else torch.complex128
    plan = make(fa, n, dtype)
    p, q, amp = 12345, (n // 3) | 1, 0.5
    k = torch.arange(n, device="cuda", dtype=torch.int64)
    ang = (2.0 * np.pi / n) * torch.remainder(k * q, n).double()   # tone at bin q (k*q < 2^63: exact in int64)
    x = torch.empty(n, dtype=cdt, device="cuda")
    x.real = (amp * torch.cos(ang)).to(x.real.dtype)
    x.imag = (amp * torch.sin(ang)).to(x.real.dtype)
    x[p] += 1.0
    del ang
    y = torch.empty_like(x)
    plan.transform(x.view(1, n), y.view(1, n), fa.Transform.Fft)
    torch.cuda.synchronize()
    ang = (-2.0 * np.pi / n) * torch.remainder(k * p, n).double()  # impulse at p -> exp(-2 pi i p k / n)
    del k
    err2 = ((y.real.double() - torch.cos(ang)) ** 2).sum()
    err2 += ((y.imag.double() - torch.sin(ang)) ** 2).sum()
    del ang
    # the tone adds amp*n at bin q: remove it from the error sum analytically
    yq = complex(y[q].item())
    ph = -2.0 * np.pi * ((p * q) % n) / n
    model_q = complex(np.cos(ph), np.sin(ph))
    err2 = float(err2) - abs(yq - model_q) ** 2 + abs(yq - (model_q + amp * n)) ** 2
    ref2 = float(n) + (amp * n) ** 2
    assert np.sqrt(err2 / ref2) <= tol, (log2n, np.sqrt(err2 / ref2))
    plan.transform_in_place(y.view(1, n), fa.Transform.Ifft)
    torch.cuda.synchronize()
    d = torch.view_as_real(y - x).double().pow(2).sum().sqrt() / torch.view_as_real(x).double().pow(2).sum().sqrt()
    assert float(d) <= 2 * tol, (log2n, float(d))
    del x, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,batch,dtype,tol", [(1 << 20, 40, np.complex64, 1e-6), (4096, 70000, np.complex64, 1e-6),
                                               (999983, 20, np.complex64, 2e-6), (1 << 18, 70, np.complex128, 5e-14)])
def test_host_batched_entry_point(torch, fa, oracle, n, batch, dtype, tol):
    """Host arrays of many transforms streamed through the device in chunks (several chunks in every case here):
    identical to the device-resident batched result, sampled transforms against the oracle, in place too."""
    rng = np.random.default_rng(n + batch)
    x = (rng.random((batch, n), dtype=np.float32 if dtype == np.complex64 else np.float64)
         + 1j * rng.random((batch, n), dtype=np.float32 if dtype == np.complex64 else np.float64)).astype(dtype)
    plan = make(fa, n, dtype)
    y = np.empty_like(x)
    plan.transform_batch_host(x, y, fa.Transform.Fft)
    for b in (0, batch // 2, batch - 1):
        ref = oracle.transform_batch(x[b:b + 1], oracle.FFT)
        assert rel_l2(y[b], ref[0]) <= tol, (n, b, rel_l2(y[b], ref[0]))
    sl = slice(0, batch, max(1, batch // 16))
    assert np.array_equal(gpu_batch(torch, fa, plan, x[sl], 0), y[sl])
    z = x.copy()
    plan.transform(z, z, fa.Transform.Fft)
    assert np.array_equal(z, y)


def test_host_batched_entry_point_with_pinned_buffers(torch, fa):
    """Page-locked user buffers (torch pinned tensors) behave like pageable ones: pinned input only, pinned output
    only, both, in place.  (DMA straight from / to a large pinned user buffer was measured slower than staging
    through the four reused 32 MiB buffers -- 28.8 vs 35-40 GB/s each way -- so every buffer takes the staged route.)"""
    n, batch = 1 << 16, 300  # 150 MiB: five chunks, every slot reused
    plan = make(fa, n, np.complex64)
    rng = np.random.default_rng(5)
    x = (rng.random((batch, n), dtype=np.float32) + 1j * rng.random((batch, n), dtype=np.float32)).astype(np.complex64)
    ref = np.empty_like(x)
    plan.transform_batch_host(x, ref, fa.Transform.Fft)
    xp = torch.empty((batch, n), dtype=torch.complex64, pin_memory=True)
    yp = torch.empty((batch, n), dtype=torch.complex64, pin_memory=True)
    xp.copy_(torch.from_numpy(x))
    for xin, yout in ((xp.numpy(), np.empty_like(x)), (x, yp.numpy()), (xp.numpy(), yp.numpy())):
        yout[...] = 0
        plan.transform_batch_host(xin, yout, fa.Transform.Fft)
        assert np.array_equal(yout, ref)
    plan.transform_batch_host(xp.numpy(), xp.numpy(), fa.Transform.Fft)  # in place on pinned memory
    assert np.array_equal(xp.numpy(), ref)


def test_independent_plans_on_concurrent_host_threads(torch, fa, oracle):
    """Handles are Send, not Sync (autosort/mod.rs:54): one thread at a time per handle, but distinct handles are fully
    independent.  Four host threads, each with its own plan and its own stream, hammer the library concurrently
    (ctypes drops the GIL around the calls); every result must match the single-threaded one."""
    import threading

    sizes = [1 << 16, 40001, 4096, 729]
    xs = {n: np.stack([hash_uniform(300 + b, n) for b in range(4)]).astype(np.complex64) for n in sizes}
    refs = {n: gpu_batch(torch, fa, make(fa, n, np.complex64), xs[n], 0) for n in sizes}
    errors = []

    def worker(n):
        try:
            plan = make(fa, n, np.complex64)
            stream = torch.cuda.Stream()
            d = torch.from_numpy(xs[n]).cuda()
            o = torch.empty_like(d)
            for _ in range(40):
                with torch.cuda.stream(stream):
                    plan.transform(d, o, fa.Transform.Fft)
            stream.synchronize()
            if not np.array_equal(o.cpu().numpy(), refs[n]):
                errors.append(("mismatch", n))
        except Exception as e:  # surfaced in the main thread below
            errors.append((repr(e), n))

    threads = [threading.Thread(target=worker, args=(n,)) for n in sizes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_linearity(torch, fa):
    n = 1 << 20
    plan = make(fa, n, np.complex64)
    a = hash_uniform(1, n).astype(np.complex64)[None, :]
    b = hash_uniform(2, n).astype(np.complex64)[None, :]
    fa_, fb = gpu_batch(torch, fa, plan, a, 0), gpu_batch(torch, fa, plan, b, 0)
    fab = gpu_batch(torch, fa, plan, a + 2 * b, 0)
    assert rel_l2(fab, fa_.astype(np.complex128) + 2 * fb.astype(np.complex128)) <= 1e-6


def test_runs_on_a_side_stream(torch, fa, oracle):
    n = 1 << 16
    plan = make(fa, n, np.complex64)
    x = np.stack([hash_normal(5 + b, n) for b in range(4)]).astype(np.complex64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.from_numpy(x).cuda()
        o = torch.empty_like(d)
        plan.transform(d, o, fa.Transform.Fft)
    s.synchronize()
    assert rel_l2(o.cpu().numpy(), oracle.transform_batch(x, 0)) <= 1e-6


def test_batched_transform_is_graph_capturable(torch, fa, oracle):
    """After a warm-up call (which sizes the plan's scratch), the batched entry point is pure stream-ordered
    launches: it can be captured into a HIP graph and replayed on new data (pow2 two-pass, one-launch and
    Bluestein conv plans)."""
    for n in (1 << 16, 4096, 40001):
        plan = make(fa, n, np.complex64)
        x0 = np.stack([hash_uniform(900 + b, n) for b in range(3)]).astype(np.complex64)
        x1 = np.stack([hash_uniform(950 + b, n) for b in range(3)]).astype(np.complex64)
        d = torch.from_numpy(x0).cuda()
        o = torch.empty_like(d)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            plan.transform(d, o, fa.Transform.Fft)  # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            plan.transform(d, o, fa.Transform.Fft)
        d.copy_(torch.from_numpy(x1).cuda())
        g.replay()
        torch.cuda.synchronize()
        ref = oracle.transform_batch(x1, 0, nthreads=2)
        assert rel_l2(o.cpu().numpy(), ref) <= 2e-6, n


@pytest.mark.parametrize("src,cc,std", [("consumer.c", "gcc", "-std=c11"), ("consumer.cpp", "g++", "-std=c++14")])
def test_c_and_cxx_consumers_relink_unchanged(fa, tmp_path, src, cc, std):
    """existing C / C++ users of fourier.h build against include/fourier.h with
    -Wall -Wextra -pedantic -Werror (fourier-ffi/CMakeLists.txt:12) and link libfourier.so."""
    import subprocess

    from fourier_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", src), "-o", exe, "-L", libdir, "-l:libfourier.so",
                           "-lm", f"-Wl,-rpath,{libdir}"])
    if not os.path.exists(os.path.join(libdir, "libfourier.so.0")):  # the SONAME link a package would install
        os.symlink(_lib.LIB_PATH, str(tmp_path / "libfourier.so.0"))
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:{tmp_path}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "Tests ran successfully." in out.stdout, out.stderr[-2000:]


def _build_and_run_c(tmp_path, src, cc, std, static):
    import subprocess

    from fourier_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / (os.path.splitext(src)[0] + ("_static" if static else "")))
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "c", src), "-o", exe]
    if static:  # the archive carries the gfx950 code object; its only dependencies are the HIP runtime and libstdc++
        cmd += [os.path.join(libdir, "libfourier.a"), "-L/opt/rocm/lib", "-lamdhip64", "-lstdc++", "-lm", "-lpthread",
                "-Wl,-rpath,/opt/rocm/lib"]
    else:
        cmd += ["-L", libdir, "-l:libfourier.so", "-lm", f"-Wl,-rpath,{libdir}"]
    subprocess.check_call(cmd)
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "Tests ran successfully." in out.stdout, (out.returncode, out.stderr[-2000:])
    if static:
        needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True).stdout
        assert "libfourier" not in needed, "the static consumer must not depend on libfourier.so"


@pytest.mark.parametrize("static", [False, True])
def test_c_programs_issue_the_rust_shims_ffi_sequence(fa, tmp_path, static):
    """rust/fourier-hip cannot be compiled in this image; tests/c/ffi_sequence.c makes exactly its FFI calls
    (create -> transform_in_place -> transform -> last_status -> batch_host -> reserve -> destroy, both precisions,
    every transform code, the NULL / unknown-code / size-0 cases) against the shared library and the static archive."""
    _build_and_run_c(tmp_path, "ffi_sequence.c", "gcc", "-std=c11", static)


@pytest.mark.parametrize("src,cc,std", [("consumer.c", "gcc", "-std=c11"), ("consumer.cpp", "g++", "-std=c++14")])
def test_c_and_cxx_consumers_link_the_static_archive(fa, tmp_path, src, cc, std):
    """fourier-ffi/CMakeLists.txt:94-111 registers four ctest programs: the C and the C++ consumer, each against the
    shared and the static library.  The shared pair is test_c_and_cxx_consumers_relink_unchanged; this is the static pair."""
    _build_and_run_c(tmp_path, src, cc, std, True)


def test_error_behaviour(torch, fa):
    from fourier_amd import _lib

    L = _lib.lib()
    assert not L.fourier_create_float(0)
    L.fourier_destroy_float(None)
    x = hash_normal(3, 8).astype(np.complex64)
    buf = x.copy()
    h = L.fourier_create_float(8)
    L.fourier_transform_in_place_float(h, buf.ctypes.data, 9)  # unknown code: silent no-op
    assert np.array_equal(buf, x)
    L.fourier_transform_in_place_float(None, buf.ctypes.data, 0)  # NULL handle: no-op
    assert np.array_equal(buf, x)
    L.fourier_destroy_float(h)
    with pytest.raises(fa.FourierError):
        fa.create_fft_f32(0)
    plan = fa.create_fft_f32(8)
    with pytest.raises(ValueError):
        plan.transform(torch.zeros(12, dtype=torch.complex64, device="cuda"),
                       torch.zeros(12, dtype=torch.complex64, device="cuda"), fa.Transform.Fft)
    with pytest.raises(TypeError):
        plan.fft_in_place(torch.zeros(8, dtype=torch.complex128, device="cuda"))
    # empty batch: a successful no-op for every plan family
    for n, opts in ((8, ()), (4096, ()), (1 << 16, ()), (96, ()), (3 * 4096, ()), (100, ()), (102, ()), (40001, ())):
        p = fa.create_fft_f32(n)
        for k, v in opts:
            p.set_option(k, v)
        buf = torch.full((n,), 7 + 7j, dtype=torch.complex64, device="cuda")
        assert L.fourier_hip_transform_batch_float(p._h, buf.data_ptr(), buf.data_ptr(), 0, 0, None) == 0, n
        assert L.fourier_hip_reserve_float(p._h, 0, 1) == 0
        torch.cuda.synchronize()
        assert bool((buf == 7 + 7j).all()), n


def test_cmake_package_builds_and_its_ctest_programs_pass(torch, tmp_path):
    """packaging/CMakeLists.txt end to end on the GPU box: configure, build (the engine once more: shared library with
    SONAME libfourier.so.0, static archive, five consumer programs with -Wall -Wextra -pedantic -Werror) and `ctest` --
    what fourier-ffi/CMakeLists.txt:38-111 does for the reference.  About two minutes of compilation."""
    import shutil
    import subprocess

    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("cmake / ROCm clang not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b = str(tmp_path / "b")
    r = subprocess.run(["cmake", "-S", os.path.join(root, "packaging"), "-B", b, "-DCMAKE_HIP_COMPILER=/opt/rocm/lib/llvm/bin/clang++",
                        "-DCMAKE_PREFIX_PATH=/opt/rocm", "-DCMAKE_BUILD_TYPE=Release"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["cmake", "--build", b, "-j", "8"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(os.path.join(b, "libfourier.so.0")) and os.path.exists(os.path.join(b, "libfourier.a"))
    soname = subprocess.run(["readelf", "-d", os.path.join(b, "libfourier.so.0")], capture_output=True, text=True).stdout
    assert "libfourier.so.0" in soname
    r = subprocess.run(["ctest", "--test-dir", b, "--output-on-failure"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "100% tests passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    # the install tool refuses an argument that is not wholly a length before it touches the library (strtoull alone reads "abc" as 0
    # and "12x" as 12); 0 is a list of one length that no plan takes, not an endless loop
    for bad in ("abc", "12x", "-3", ""):
        r = subprocess.run([os.path.join(b, "fourier_warm_cache"), "1001", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "is not a length" in r.stderr and not r.stdout, (bad, r.returncode, r.stdout, r.stderr)
    r = subprocess.run([os.path.join(b, "fourier_warm_cache"), "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "1 lengths, 0 plans" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("n,family,per_block", [(8, "tiny_shfl", 256), (16, "tiny_shfl", 256), (32, "tiny_shfl", 256),
                                                (64, "rows", 32), (256, "rows", 32), (1024, "rows", 16),
                                                (96, "mixed_radix_ct", 10), (729, "mixed_radix_ct", 1)])
def test_million_transform_grids_of_the_small_n_kernels_are_value_checked(torch, fa, oracle, n, family, per_block):
    """The lane-per-transform, ROWS and LDS mixed-radix kernels at batch 2^20 + 37 (a grid of 4 thousand to a million
    workgroups with a ragged last one): >= 64 transforms sampled across the batch -- the first and last workgroup, both
    sides of workgroup boundaries far into the grid, the ragged tail, and a random scatter -- against the oracle
    (integrity.rs:145-192 is the reference's only check of these sizes, at batch 1).  Every other transform is covered
    by Parseval.  Mixed-radix lengths must match bit for bit."""
    batch = (1 << 20) + 37
    g = torch.Generator(device="cuda")
    g.manual_seed(4242 + n)
    x = torch.empty((batch, n), dtype=torch.complex64, device="cuda")
    torch.view_as_real(x).normal_(0.0, 1.0, generator=g)
    y = torch.full_like(x, float("nan"))
    plan = make(fa, n, np.complex64)
    plan.transform(x, y, fa.Transform.Fft)
    torch.cuda.synchronize()
    rng = np.random.default_rng(n)
    blocks = [0, 1, 2, 1000, 4097, (batch // per_block) // 2, batch // per_block - 1]
    idx = set(range(8)) | set(range(batch - 40, batch)) | set(int(i) for i in rng.integers(0, batch, 24))
    for b in blocks:  # last transform of one workgroup, first of the next
        idx |= {min(batch - 1, max(0, b * per_block + d)) for d in (-1, 0, 1, per_block - 1, per_block)}
    idx = sorted(idx)
    assert len(idx) >= 64
    sel = torch.tensor(idx, device="cuda")
    hx, hy = x[sel].cpu().numpy(), y[sel].cpu().numpy()
    ref = oracle.transform_batch(hx, oracle.FFT)
    if family == "mixed_radix_ct":
        assert np.array_equal(hy, ref.astype(np.complex64)), (n, plan.describe())
    else:
        for k, i in enumerate(idx):
            assert rel_l2(hy[k], ref[k]) <= 1e-6, (n, i, plan.describe(), rel_l2(hy[k], ref[k]))
    # Parseval over the whole batch, per transform: sum |X|^2 = n * sum |x|^2
    ex = (torch.view_as_real(x) ** 2).sum(dim=(1, 2), dtype=torch.float64)
    ey = (torch.view_as_real(y) ** 2).sum(dim=(1, 2), dtype=torch.float64)
    assert bool(torch.isfinite(ey).all())
    assert float(((ey - n * ex).abs() / (n * ex)).max()) <= 2e-5, n



@pytest.mark.parametrize("n,dtype,tol", [(999983, np.complex64, 2e-6), (65537, np.complex64, 2e-6), (2200000, np.complex64, 2e-6),
                                         (999983, np.complex128, 1e-9), (70001, np.complex128, 5e-11)])
def test_bluestein_chirp_in_pass_computes_the_chirp(torch, fa, oracle, n, dtype, tol):
    """Option bluestein_chirp_compute (default on): the chirp-in first pass builds exp(-i*pi*k^2/N) from a row table, a
    column table and an exact-exponent cross term instead of reading the N-entry table (a quarter of that pass's
    HBM-side traffic).  Against the oracle and against the table-reading route, forward and inverse."""
    x = np.stack([hash_uniform(880 + b, n) for b in range(2)]).astype(dtype)
    comp, read = make(fa, n, dtype), make(fa, n, dtype)
    for p in (comp, read):
        p.set_option("bluestein_smooth_m", 0)  # (the smooth-M route reads the chirp table)
    comp.set_option("bluestein_chirp_compute", 1)  # the default turns it on only for long first passes and large tables
    read.set_option("bluestein_chirp_compute", 0)
    for code in (0, 1, 3):
        ref = oracle.transform_batch(x, code)
        a, b = gpu_batch(torch, fa, comp, x, code), gpu_batch(torch, fa, read, x, code)
        assert rel_l2(a, ref) <= tol and rel_l2(b, ref) <= tol, (n, code, rel_l2(a, ref), rel_l2(b, ref))
        assert rel_l2(a, b) <= (4e-7 if dtype == np.complex64 else 1e-12), (n, code, rel_l2(a, b))
        assert np.array_equal(gpu_batch(torch, fa, comp, x, code, inplace=True), a), (n, code)


@pytest.mark.parametrize("n,dtype,tol", [(59049, np.complex64, 1e-6), (62208, np.complex64, 1e-6), (39366, np.complex64, 1e-6),
                                         (55296, np.complex64, 1e-6), (20736, np.complex64, 1e-6), (2 * 3 ** 13, np.complex64, 1e-6),
                                         (10368, np.complex128, 5e-14), (13122, np.complex128, 5e-14), (2048 * 3 ** 9, np.complex128, 5e-14)])
def test_mixed_radix_sizes_beyond_the_lds_limit_with_a_small_power_of_two(torch, fa, fa_exp, oracle, monkeypatch, n, dtype, tol):
    """2^a * 3^b with a < 12 above the LDS kernels' 19683 (f32) / 9216 (f64) points: two or three big-radix passes of mixed
    length on column tiles (kernels_tiled.h, round 4) -- and, for the rare length without such a factorisation and as the A/B
    arm of the experiments library, the reference's Stockham pass by pass in global memory (stockham_pass_kernel, radices
    27 / 9 / 3 then 16 / 8 / 4 / 2).  All five codes, in and out of place, a ragged batch, ragged tiles, against the oracle."""
    batch = 5 if n < 1 << 20 else 2
    x = np.stack([hash_normal(1900 + b, n) for b in range(batch)]).astype(dtype)
    for route in ("mixed tiles", "global-pass"):
        if route == "global-pass":
            monkeypatch.setenv("FOURIER_NO_TILED_MIXED", "1")  # honoured by the experiments library only (fa_exp is bound)
        plan = make(fa, n, dtype)
        assert route in plan.describe(), plan.describe()
        for code in range(5):
            ref = oracle.transform_batch(x, code)
            assert rel_l2(gpu_batch(torch, fa, plan, x, code), ref) <= tol, (n, code, route)
            assert rel_l2(gpu_batch(torch, fa, plan, x, code, inplace=True), ref) <= tol, (n, code, route, "in place")


@pytest.mark.parametrize("n", [5, 35, 77, 125, 143, 350, 625, 1000, 1001, 2401, 3125, 4095, 5005, 8008, 9009, 9100, 10000, 15625, 16807, 20000, 20480])
def test_lengths_with_prime_factors_5_to_13_run_as_stockham_passes(torch, fa, oracle, n):
    """Beyond the reference (which sends them to Bluestein, fourier/src/lib.rs:38-42): lengths whose prime factors stop at
    13 run the LDS Stockham kernel with the radix list continued [4,8,4,3,2,5,7,11,13] -- per-length kernels for the
    reference's own 5^k benchmark lengths and round decimal lengths, the runtime-parameterised kernel otherwise.  All
    codes, in and out of place, a ragged batch over many workgroups; within the Bluestein tolerance of the oracle and,
    being a direct factorisation, tighter against f64 truth.  Round 6 (sessions 49 - 51): where regfft_shapes.h lists the length in the
    precision, the transform runs on two or three register stages in one launch instead (kernels_regfft.h)."""
    batch = max(3, min(4099, (1 << 19) // n)) | 1
    x = np.stack([hash_normal(2100 + (b % 7), n) for b in range(7)])
    for dtype, tl2, ttruth in ((np.complex64, 2e-6, 4e-7), (np.complex128, 5e-11, 3e-15)):
        plan = make(fa, n, dtype)
        m = n
        while m % 2 == 0 or m % 3 == 0 or m % 5 == 0:
            m //= 2 if m % 2 == 0 else (3 if m % 3 == 0 else 5)
        per_length = (m == 1 or n in (49, 343, 2401, 16807)) and n * np.dtype(dtype).itemsize <= 160 * 1024  # 2^a*3^b*5^c, 7^k
        f64_wide_13 = dtype == np.complex128 and n > 2048 and (n % 11 == 0 or n % 13 == 0)  # does not fit the registers
        if regfft_shape(n, dtype):
            assert plan.describe().startswith(f"stockham registers {regfft_shape(n, dtype)} one-launch"), plan.describe()
        elif not per_length and (n > 8192 or f64_wide_13):  # the runtime-parameterised kernel stops at 8192 points
            m7 = n
            while m7 % 2 == 0 or m7 % 3 == 0 or m7 % 5 == 0 or m7 % 7 == 0:
                m7 //= 2 if m7 % 2 == 0 else (3 if m7 % 3 == 0 else (5 if m7 % 5 == 0 else 7))
            def _s7(v):
                for p in (2, 3, 5, 7):
                    while v % p == 0:
                        v //= p
                return v == 1
            menu = [L for L in range(64, 513) if _s7(L)]
            tiles2 = any(n % a == 0 and 64 <= n // a <= a and _s7(n // a) for a in menu)
            tiles3 = any(n % a == 0 and (n // a) % b == 0 and 64 <= n // a // b <= b <= a and _s7(n // a // b) for a in menu for b in menu)
            if m7 != 1 or not (tiles2 or tiles3):  # a factor 11 / 13 beyond the LDS kernels, or no split into tile lengths (f64 7^5 = 343 x 49)
                assert "bluestein" in plan.describe(), plan.describe()
                continue
            # round 5: prime factors up to 7 beyond the LDS kernels -- ahead-of-time tile passes (f64 15625 = 125 x 125, 20480 = 160 x 128)
            assert plan.describe().startswith("stockham mixed tiles"), plan.describe()
        else:
            assert plan.describe().startswith("stockham mixed-radix"), plan.describe()
        xs = np.tile(x.astype(dtype), ((batch + 6) // 7, 1))[:batch]
        truth = np.fft.fft(x.astype(np.complex128), axis=1)
        for code in range(5):
            ref = oracle.transform_batch(xs[:7], code)
            got = gpu_batch(torch, fa, plan, xs, code)
            assert rel_l2(got[:7], ref) <= tl2, (n, code, rel_l2(got[:7], ref))
            assert all(np.array_equal(got[b], got[b % 7]) for b in range(7, batch)), (n, code)  # every workgroup, same bits
            assert np.array_equal(gpu_batch(torch, fa, plan, xs, code, inplace=True), got), (n, code)
        assert rel_l2(gpu_batch(torch, fa, plan, xs[:7], 0), truth) <= ttruth, n


@pytest.mark.parametrize("dtype,log2n", [(np.complex64, 29), (np.complex128, 28)])
def test_a_single_transform_of_4_gib_addresses_correctly(torch, fa, dtype, log2n):
    """One transform of 4 GiB (f32 2^29, f64 2^28; three passes): every byte offset beyond 32 bits.  The column-tile
    accesses go through buffer descriptors whose 64-bit base carries the row and whose lane offset stays below
    n * sizeof(complex) / 16 (fft_kernels.h, pass_tile), so no size limit applies -- checked with a known answer: two
    complex tones give two spectral lines (N and N/2 high) and nothing else, in and out of place, forward and back."""
    n = 1 << log2n
    cdt = torch.complex64 if dtype == np.complex64 else torch.complex128
    rdt = torch.float32 if dtype == np.complex64 else torch.float64
    f1, f2 = 123456789 % n, n - 7
    x = torch.empty(n, dtype=cdt, device="cuda")
    xr = torch.view_as_real(x)
    step = 1 << 24
    for lo in range(0, n, step):  # exact phases: (f * k mod n) / n in f64
        k = torch.arange(lo, lo + step, device="cuda", dtype=torch.int64)
        p1 = ((k * f1) % n).double() * (2.0 * np.pi / n)
        p2 = ((k * f2) % n).double() * (2.0 * np.pi / n)
        xr[lo:lo + step, 0] = (torch.cos(p1) + 0.5 * torch.cos(p2)).to(rdt)
        xr[lo:lo + step, 1] = (torch.sin(p1) + 0.5 * torch.sin(p2)).to(rdt)
    del k, p1, p2
    plan = make(fa, n, dtype)
    assert plan.describe().count("x") == 2, plan.describe()  # three passes
    y = torch.empty_like(x)
    plan.transform(x.view(1, n), y.view(1, n), fa.Transform.Fft)
    torch.cuda.synchronize()
    eps = 2e-5 if dtype == np.complex64 else 1e-11
    for out in (y,):
        mag = out.abs()
        assert abs(float(mag[f1]) / n - 1.0) < eps and abs(float(mag[f2]) / n - 0.5) < eps
        mag[f1] = 0
        mag[f2] = 0
        assert float(mag.max()) / n < eps, float(mag.max()) / n
        del mag
    plan.transform(y.view(1, n), y.view(1, n), fa.Transform.Ifft)  # in place (through the plan's scratch), back to the tones
    torch.cuda.synchronize()
    err = float((torch.view_as_real(y) - xr).abs().max())
    assert err < (2e-5 if dtype == np.complex64 else 1e-12), err


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_a_non_finite_transform_does_not_reach_its_neighbours(torch, fa, oracle, dtype):
    """Transforms of a batch are independent (fft.rs:51-61: one plan call per transform): a row of NaN / Inf poisons its own
    output only, in every plan family -- lane-per-transform, whole rows, one-launch, LDS mixed-radix, the one-launch chirp-z
    (whose padding positions used to read the NEXT transform's row times a zero chirp) and the tiled plans."""
    for n, batch in ((8, 70), (17, 37), (64, 33), (96, 21), (127, 19), (439, 11), (625, 7), (1000, 6), (1013, 6), (4096, 5),
                     (10007, 4), (1 << 16, 3), (40009, 3)):
        x = np.stack([hash_normal(900 + b, n) for b in range(batch)]).astype(dtype)
        ref = oracle.transform_batch(x, 0)
        plan = make(fa, n, dtype)
        # f64 chirp-z of a long transform: the ORACLE's unreduced chirp angle (bluesteins.rs:10,31,57) costs it digits
        tol = 2e-6 if dtype == np.complex64 else (2e-10 if n > 4096 and "bluestein" in plan.describe() else 2e-12)
        for bad_row, bad in ((1, np.nan), (batch - 1, np.inf), (0, -np.inf)):
            xb = x.copy()
            xb[bad_row, n // 2] = bad
            got = gpu_batch(torch, fa, plan, xb, 0)
            keep = [b for b in range(batch) if b != bad_row]
            assert np.isfinite(got[keep]).all(), (n, plan.describe(), bad_row)
            assert rel_l2(got[keep], ref[keep]) <= tol, (n, plan.describe(), bad_row)
            assert not np.isfinite(got[bad_row]).all(), (n, bad_row)


def test_prefetching_last_pass_matches_the_plain_last_pass(torch, fa, fa_exp, oracle):
    """Plan option last_pass_prefetch of the EXPERIMENTS library (fft_last_prefetch_kernel): the LAST
    pass as persistent workgroups that fetch their next tile -- eight rows by LDS-DMA into the idle exchange buffer, eight into
    registers -- ahead of the current tile's stores.  Measured slower (kernels_experiments.h), so the product library does not
    carry it.  Same in-tile arithmetic as fft_pass_kernel, but another kernel: the compiler contracts the same source into
    different FMAs, so the two agree to rounding (3e-7 / 1e-15), not bit for bit -- for 2^21 (last pass of length 1024), 2^22
    (2048), f32 and f64, forward / inverse / scaled, in place, a tile count that does not divide over the resident workgroups,
    and the chirp-out pass of C4's Bluestein plan."""
    from fourier_amd import _lib

    assert "libfourier_experiments" in _lib.lib()._name
    for n, dtype, batch in ((1 << 21, np.complex64, 37), (1 << 22, np.complex64, 37), (1 << 21, np.complex128, 19), (1 << 22, np.complex128, 11),
                            (999983, np.complex64, 21), (600011, np.complex128, 5)):
        g = torch.Generator(device="cuda")
        g.manual_seed(n % 1000 + batch)
        x = torch.empty((batch, n), dtype=torch.complex64 if dtype == np.complex64 else torch.complex128, device="cuda")
        torch.view_as_real(x).normal_(0.0, 1.0, generator=g)
        on, off = make(fa, n, dtype), make(fa, n, dtype)
        on.set_option("last_pass_prefetch", 1)
        off.set_option("last_pass_prefetch", 0)
        close = 3e-7 if dtype == np.complex64 else 1e-15
        for code in (0, 1, 4):
            a, b = torch.empty_like(x), torch.empty_like(x)
            on.transform(x, a, fa.Transform(code))
            off.transform(x, b, fa.Transform(code))
            torch.cuda.synchronize()
            assert float(torch.linalg.norm(a - b) / torch.linalg.norm(b)) <= close, (n, dtype, code)
            c = x.clone()
            on.transform(c, c, fa.Transform(code))
            torch.cuda.synchronize()
            assert torch.equal(torch.view_as_real(c), torch.view_as_real(a)), (n, dtype, code, "in place")
        ref = oracle.transform_batch(x[:1].cpu().numpy(), 0)
        on.transform(x, a, fa.Transform.Fft)
        torch.cuda.synchronize()
        pow2 = n & (n - 1) == 0
        tol = (1e-6 if pow2 else 2e-6) if dtype == np.complex64 else (5e-14 if pow2 else 1e-9)
        assert rel_l2(a[:1].cpu().numpy(), ref) <= tol, (n, dtype)
        del x, a, b, c
        torch.cuda.empty_cache()


def test_lengths_with_factors_5_and_7_beyond_the_lds_kernels_run_as_tile_passes_by_default(torch, fa, oracle):
    """Round 5: tile-pass kernels for every length 64 ... 512 whose prime factors stop at 7 are compiled ahead of time, so that the
    lengths the reference sends to Bluestein (fourier/src/lib.rs:38-42) but that factor into two or three such tile lengths take
    direct Stockham passes from plain create_fft_*: 10^5, 44100, 48000, 96000, 10^6, f64 19600 (beyond the
    LDS limit; 9800 and f32 19600, the cases of rounds 5 / 6, run on three register stages since, regfft_shapes.h), a ragged case (tile length without a factor 16).  Values against the oracle (chirp-z) and the f64 truth."""
    for n, dtype, want in ((100000, np.complex64, "400x250"), (44100, np.complex64, "210x210"), (1000000, np.complex64, "1000x1000"), (1000000, np.complex128, "100x100x100"),
                           (48000, np.complex64, None), (96000, np.complex64, None), (19600, np.complex128, None), (30870, np.complex64, None),
                           (100000, np.complex128, "400x250"), (44100, np.complex128, "210x210"), (5 * 7 * 7 * 7 * 7 * 3, np.complex128, None),
                           # round 6: tile lengths of 513 ... 1024 points (register tiles on 64-byte rows): two passes where there were three, or Bluestein
                           (390625, np.complex64, "625x625"), (500000, np.complex128, "800x625"), (640000, np.complex64, "800x800"), (729000, np.complex128, "900x810"),
                           # f32 only: stages of up to 40 points (1000 = 40 x 25; f64 spills there and keeps three passes, r06_s42)
                           (765625, np.complex64, "875x875"), (945000, np.complex64, "1000x945")):
        plan = make(fa, n, dtype)
        d = plan.describe()
        assert "stockham mixed tiles" in d and "specialised" not in d, (n, d)
        if want:
            assert "mixed tiles " + want in d, (n, d)
        x = np.stack([hash_normal(2700 + b, n) for b in range(3)]).astype(dtype)
        tol = 2e-6 if dtype == np.complex64 else 1e-9  # f64: the ORACLE's unreduced chirp angle (bluesteins.rs:10,31,57)
        for code in range(5):
            ref = oracle.transform_batch(x, code)
            a = gpu_batch(torch, fa, plan, x, code)
            assert rel_l2(a, ref) <= tol, (n, dtype, code, rel_l2(a, ref))
            assert rel_l2(gpu_batch(torch, fa, plan, x, code, inplace=True), ref) <= tol, (n, dtype, code)
        truth = torch.fft.fft(torch.from_numpy(x).to(torch.complex128)).numpy()
        assert rel_l2(gpu_batch(torch, fa, plan, x, 0), truth) <= (4e-7 if dtype == np.complex64 else 3e-15), (n, dtype)


def test_code_object_cache_and_the_library_wide_specialise_policy(torch, fa, oracle, tmp_path, monkeypatch):
    """Round 5: a drop-in caller reaches the specialised kernels without a per-handle call.
    "specialise_at_create" = 2 (fourier_hip_set_default_option, or FOURIER_HIP_SPECIALISE=2 in the environment of a program that
    cannot be changed) compiles a length's own kernel inside create and leaves the code object in the on-disk cache; the default
    policy 1 loads it from there in any later process -- in milliseconds, without libhiprtc --, policy 0 never does; a cache file
    that cannot be loaded is discarded and compiled again.  (Round 6, sessions 49 - 51: most lengths up to 10240 points with factors 7 / 11 / 13 now
    have ahead-of-time register-stage kernels, regfft_shapes.h -- 5005, 1001, 3003 and 9009, this test's lengths until then, among them; the
    lengths here are ones that still take the runtime-parameterised kernel or Bluestein by default: 4459 = 7^3 13, 3773 = 7^3 11, 4802 = 2 7^4,
    11011 = 7 11^2 13.)"""
    import shutil
    import subprocess
    import sys

    if not (os.path.exists("/opt/rocm/lib/libhiprtc.so") or shutil.which("hipcc")):
        pytest.skip("libhiprtc not installed")
    cache = tmp_path / "co-cache"
    monkeypatch.setenv("FOURIER_HIP_CACHE_DIR", str(cache))
    prev = fa.get_default_option("specialise_at_create")
    try:
        fa.set_default_option("specialise_at_create", 0)
        assert "specialised" not in make(fa, 4459, np.complex64).describe()
        fa.set_default_option("specialise_at_create", 1)  # cache only: the cache is empty, nothing may be compiled
        assert "specialised" not in make(fa, 4459, np.complex64).describe() and not (cache.exists() and list(cache.iterdir()))
        fa.set_default_option("specialise_at_create", 2)
        for n, dtype, kind in ((4459, np.complex64, "mixed-radix"), (4802, np.complex128, "mixed-radix"), (11011, np.complex64, "mixed-radix"),
                               (57200, np.complex64, "mixed tiles")):
            plan = make(fa, n, dtype)
            assert kind in plan.describe() and "specialised" in plan.describe(), plan.describe()
            x = np.stack([hash_normal(2800 + b, n) for b in range(5)]).astype(dtype)
            assert rel_l2(gpu_batch(torch, fa, plan, x, 0), oracle.transform_batch(x, 0)) <= (2e-6 if dtype == np.complex64 else 5e-11)
        assert make(fa, 1013, np.complex64).describe().startswith("bluestein")  # not of the family: its default route, no error
        files = sorted(p.name for p in cache.iterdir())
        assert len(files) == 5 and all(f.endswith(".co") and "gfx950" in f for f in files), files  # 57200 = 260 x 220: two tile kernels
        with pytest.raises(fa.FourierError):
            fa.set_default_option("specialise_at_create", 3)
        with pytest.raises(fa.FourierError):
            fa.set_default_option("no_such_key", 1)
    finally:
        fa.set_default_option("specialise_at_create", prev)
    # later processes: the default policy (no variable), policy 0, policy 2 on a length the cache does not hold; timing of a cache hit
    prog = ("import os, sys, time, json; sys.path.insert(0, %r); import fourier_amd as fa\n"
            "fa.create_fft_f32(4096)\n"  # the HIP runtime and the library are up before the clock starts
            "t0 = time.perf_counter(); p = fa.create_fft_f32(4459); dt = time.perf_counter() - t0\n"
            "print(json.dumps({'d4459': p.describe(), 'create_s': dt, 'd3773': fa.create_fft_f32(3773).describe(), 'policy': fa.get_default_option('specialise_at_create')}))\n"
            % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    def child(policy):
        env = {k: v for k, v in os.environ.items() if k != "FOURIER_HIP_SPECIALISE"}
        env["FOURIER_HIP_CACHE_DIR"] = str(cache)
        if policy is not None:
            env["FOURIER_HIP_SPECIALISE"] = policy
        out = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])
    r = child(None)
    assert r["policy"] == 1 and "specialised" in r["d4459"] and "specialised" not in r["d3773"], r
    assert r["create_s"] < 0.6, r  # a cache hit: read 1 file, load 1 module (a compilation takes a second or more; loose: a loaded box)
    r = child("0")
    assert r["policy"] == 0 and "specialised" not in r["d4459"], r
    r = child("2")
    assert "specialised" in r["d4459"] and "specialised" in r["d3773"], r
    # a cache directory that cannot be created, or none at all (empty variable): compilation still works, nothing is cached
    for bad in ("/proc/fourier-hip-no-such-dir/x", ""):
        env = {k: v for k, v in os.environ.items() if k != "FOURIER_HIP_SPECIALISE"}
        env.update(FOURIER_HIP_CACHE_DIR=bad, FOURIER_HIP_SPECIALISE="2")
        out = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "specialised" in json.loads(out.stdout.strip().splitlines()[-1])["d4459"], (bad, out.stdout)
    # a cache file somebody else could have written is not trusted (a code object runs on the device): ignored, left alone
    victim = next(p for p in cache.iterdir() if "-n4459-" in p.name)
    victim.chmod(0o666)
    r = child(None)
    assert "specialised" not in r["d4459"] and victim.exists(), r
    victim.chmod(0o600)
    assert "specialised" in child(None)["d4459"]
    # ... nor is an entry in a directory somebody else may write, nor one behind a symbolic link (another user of a shared
    # cache directory could link one of the victim's own entries under another length's name -- a wrong-length kernel would then run out
    # of bounds on the device); an entry also names its own key, so a renamed copy is refused (and discarded: the file is ours)
    cache.chmod(0o777)
    assert "specialised" not in child(None)["d4459"]
    cache.chmod(0o700)
    assert "specialised" in child(None)["d4459"]
    other = next(p for p in cache.iterdir() if "-n11011-" in p.name)
    good = victim.read_bytes()
    victim.unlink()
    victim.symlink_to(other)
    r = child(None)
    assert "specialised" not in r["d4459"] and victim.is_symlink(), r
    victim.unlink()
    victim.write_bytes(other.read_bytes())  # a well-formed entry of ANOTHER length under this name
    victim.chmod(0o600)
    r = child(None)
    assert "specialised" not in r["d4459"] and not victim.exists(), r
    victim.write_bytes(good[:-7])  # truncated
    victim.chmod(0o600)
    r = child(None)
    assert "specialised" not in r["d4459"] and not victim.exists(), r
    # a damaged cache file (here: the format of round 5) is discarded, not trusted
    victim.write_bytes(b"FOURIER-HIP-CO-1\nnot_a_kernel\n" + b"\x00" * 100)
    victim.chmod(0o600)
    fa.set_default_option("specialise_at_create", 1)
    try:
        # the process cache still holds the kernel of this process; a fresh process must fall back to its default route, silently
        r = child(None)
        assert "specialised" not in r["d4459"] and not victim.exists(), r
    finally:
        fa.set_default_option("specialise_at_create", prev)
    # the install step (packaging/warm_cache.c, python -m fourier_amd.warm_cache): after it, a plain create of a length with factors
    # 7 / 11 / 13 runs on its own kernel -- f64 4459 leaves Bluestein -- in a process that never heard of any option
    env = {k: v for k, v in os.environ.items() if k != "FOURIER_HIP_SPECIALISE"}
    env["FOURIER_HIP_CACHE_DIR"] = str(tmp_path / "warm")
    out = subprocess.run([sys.executable, "-m", "fourier_amd.warm_cache", "4459", "4802", "3773"], env=env, capture_output=True, text=True, timeout=600,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "6 plans run on kernels of their own" in out.stdout, (out.stdout, out.stderr[-1500:])
    prog2 = ("import sys, json; sys.path.insert(0, %r); import fourier_amd as fa\n"
             "print(json.dumps([fa.create_fft_f32(4459).describe(), fa.create_fft_f64(4459).describe(), fa.create_fft_f64(4802).describe()]))\n"
             % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", prog2], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ds = json.loads(out.stdout.strip().splitlines()[-1])
    assert all("specialised" in d and not d.startswith("bluestein") for d in ds), ds


def test_plan_option_specialise_compiles_the_lengths_own_kernel_with_hiprtc(torch, fa, oracle):
    """Plan option "specialise" (rtc.cpp): a length whose prime factors stop at 13 but that has no ahead-of-time per-length
    kernel gets mixed_radix_kernel_ct<T, n> compiled with hipRTC on request.  Lengths on the runtime-parameterised kernel
    (f32 175, 4459, 3773; f64 4802), lengths beyond its reach that default to Bluestein (11011 f32, 4459 f64, 15015 f32 = 117 KiB of
    LDS), lengths that already have a kernel of their own (1000: per-length LDS kernel; 1001, 5005: register stages, regfft_shapes.h, round 6 --
    OK, unchanged), and lengths outside the family (1013, 2^12: UNSUPPORTED, the plan keeps working).  Values against the oracle and
    against the plan's default route."""
    import shutil

    if not (os.path.exists("/opt/rocm/lib/libhiprtc.so") or shutil.which("hipcc")):
        pytest.skip("libhiprtc not installed")
    for n, dtype in ((175, np.complex64), (4459, np.complex64), (3773, np.complex64), (11011, np.complex64), (15015, np.complex64),  # 15015: 117 KiB of (static) LDS
                     (4802, np.complex128), (4459, np.complex128), (1000, np.complex64), (1001, np.complex64), (5005, np.complex128)):
        batch = 37
        x = np.stack([hash_normal(2500 + b, n) for b in range(batch)]).astype(dtype)
        base, spec = make(fa, n, dtype), make(fa, n, dtype)
        before = spec.describe()
        spec.set_option("specialise", 1)
        after = spec.describe()
        if n in (1000, 1001, 5005):
            assert after == before and "specialised" not in after  # already a per-length kernel
            assert ("registers" in after) == (n != 1000), after
        else:
            assert "mixed-radix" in after and "specialised" in after, (n, before, after)
        tol = 2e-6 if dtype == np.complex64 else 5e-11
        for code in range(5):
            ref = oracle.transform_batch(x, code)
            a = gpu_batch(torch, fa, spec, x, code)
            assert rel_l2(a, ref) <= tol, (n, dtype, code, rel_l2(a, ref))
            assert rel_l2(gpu_batch(torch, fa, base, x, code), a) <= tol, (n, dtype, code)
            assert np.array_equal(gpu_batch(torch, fa, spec, x, code, inplace=True), a), (n, dtype, code)
    # beyond one compute unit's LDS: column-tile passes whose lengths may have prime factors up to 13 (Bluestein by default where a
    # tile length has a factor 11 or 13: the ahead-of-time tile kernels stop at 7)
    # (286000 = 2^4 * 5^3 * 11 * 13: tile passes of more than 512 points compiled at run time -- 500000 and 5^8, the cases of round 5, have
    # ahead-of-time register-tile kernels since round 6)
    for n, dtype, want in ((143000, np.complex64, "440x325"), (57200, np.complex64, "260x220"),
                           (143000, np.complex128, "440x325"), (286000, np.complex64, "550x520"), (286000, np.complex128, "550x520")):
        x = np.stack([hash_normal(2600 + b, n) for b in range(3)]).astype(dtype)
        base, spec = make(fa, n, dtype), make(fa, n, dtype)
        assert "bluestein" in base.describe()
        spec.set_option("specialise", 1)
        assert "mixed tiles " + want + " specialised" in spec.describe(), spec.describe()
        tol = 2e-6 if dtype == np.complex64 else 1e-9  # f64: the ORACLE's unreduced chirp angle (bluesteins.rs:10,31,57)
        for code in (0, 1, 4):
            ref = oracle.transform_batch(x, code)
            a = gpu_batch(torch, fa, spec, x, code)
            assert rel_l2(a, ref) <= tol, (n, dtype, code, rel_l2(a, ref))
            assert rel_l2(gpu_batch(torch, fa, spec, x, code, inplace=True), ref) <= tol, (n, dtype, code)
        truth = torch.fft.fft(torch.from_numpy(x).to(torch.complex128)).numpy()
        assert rel_l2(gpu_batch(torch, fa, spec, x, 0), truth) <= (4e-7 if dtype == np.complex64 else 3e-15), (n, dtype)
    # a plan on ahead-of-time tile passes has nothing to specialise: OK, unchanged
    plan = make(fa, 100000, np.complex64)
    desc = plan.describe()
    plan.set_option("specialise", 1)
    assert plan.describe() == desc and "specialised" not in desc
    for n in (1013, 17017, 4096, 999983):  # not of the family (17017 = 17 * 1001): refused, and the plan is untouched
        plan = make(fa, n, np.complex64)
        desc = plan.describe()
        with pytest.raises(fa.FourierError):
            plan.set_option("specialise", 1)
        assert plan.describe() == desc
        x = hash_normal(7, n).astype(np.complex64)[None, :]
        assert rel_l2(gpu_batch(torch, fa, plan, x, 0), oracle.transform_batch(x, 0)) <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("n,dtype,desc,tol", [(16411, np.complex64, "M=32928 inner mixed tiles 196x168", 2e-6), (65537, np.complex64, "M=131220 inner mixed tiles 405x324", 2e-6),
                                              (70001, np.complex64, "inner mixed tiles", 2e-6), (18221, np.complex64, "inner mixed tiles", 2e-6), (40001, np.complex64, "inner mixed tiles", 2e-6),
                                              (8209, np.complex128, "inner mixed tiles", 5e-11), (10007, np.complex128, "M=20160 inner mixed tiles 168x120", 5e-11),
                                              (20011, np.complex128, "M=40320 inner mixed tiles", 5e-11), (40001, np.complex128, "inner mixed tiles", 5e-11),
                                              (65537, np.complex128, "M=131220 inner mixed tiles 405x324", 1e-10), (80021, np.complex128, "inner mixed tiles", 1e-10)])
def test_bluestein_on_a_smooth_work_array(torch, fa, oracle, n, dtype, desc, tol):
    """Round 6: Bluestein's M need only reach 2N - 1 (bluesteins.rs:110; the reference rounds up to a power of two, up
    to 4N).  Where the power-of-two work array is swept three times and is at least 1.6 x longer, the plan takes a product of two tile
    lengths (the smallest, or one up to 4 % longer that splits more evenly) and runs the same three sweeps on register tiles (kernels_regtile.h): every code against the oracle and the
    f64 truth, in place, a ragged batch, against the power-of-two route (plan option bluestein_smooth_m = 0) and back."""
    plan, pow2 = make(fa, n, dtype), make(fa, n, dtype)
    assert "bluestein" in plan.describe() and desc in plan.describe(), plan.describe()
    pow2.set_option("bluestein_smooth_m", 0)
    assert "mixed tiles" not in pow2.describe() and "M=%d " % (1 << int(np.ceil(np.log2(2 * n - 1)))) in pow2.describe(), pow2.describe()
    x = np.stack([hash_uniform(3300 + b, n) for b in range(5)]).astype(dtype)
    d = torch.from_numpy(x).cuda()
    o = torch.empty_like(d)
    names = [p[0] for p in plan.profile_batch_ptr(d.data_ptr(), o.data_ptr(), 5, 0, 0) if p[2] > 0]
    assert names == ["chirp_in_pass", "conv_pass", "chirp_out_pass"], names
    truth = torch.fft.fft(torch.from_numpy(x).to(torch.complex128)).numpy()
    for code in range(5):
        a = gpu_batch(torch, fa, plan, x, code)
        assert np.array_equal(gpu_batch(torch, fa, plan, x, code, inplace=True), a), (n, code)
        assert rel_l2(a, gpu_batch(torch, fa, pow2, x, code)) <= (4e-7 if dtype == np.complex64 else 4e-15), (n, code)
        if code in (0, 1, 4):
            ref = oracle.transform_batch(x, code, nthreads=2)
            assert rel_l2(a, ref) <= tol, (n, code, rel_l2(a, ref))
    assert rel_l2(gpu_batch(torch, fa, plan, x, 0), truth) <= (4e-7 if dtype == np.complex64 else 4e-15), n
    back = gpu_batch(torch, fa, plan, gpu_batch(torch, fa, plan, x, 0), 1)
    assert rel_l2(back, x) <= (6e-7 if dtype == np.complex64 else 6e-15), n
    pow2.set_option("bluestein_smooth_m", 1)
    assert pow2.describe() == plan.describe()
    assert np.array_equal(gpu_batch(torch, fa, pow2, x, 0), gpu_batch(torch, fa, plan, x, 0)), n


@pytest.mark.gpu
def test_bluestein_smooth_work_array_only_where_it_pays(torch, fa):
    """Lengths just below a power of two (M / M_smooth below 1.6), every M the one-launch kernels hold and lengths beyond the products of two
    tile lengths (M > 512 x 512) keep the reference's power of two; the option is refused on plans that are not Bluestein."""
    for n, dtype in ((24001, np.complex64), (44017, np.complex64), (100003, np.complex64), (5003, np.complex128), (12289, np.complex128),
                     (90001, np.complex128), (999983, np.complex64)):
        d = make(fa, n, dtype).describe()
        assert "bluestein" in d and "mixed tiles" not in d, (n, d)
    # short lengths: f64 takes the register route wherever its menu reaches (2N - 1 <= 1024), f32 only where that M is a tenth shorter than the
    # power of two (or up to 64 points) -- the reference's own bench sizes 222 and 439 (fft_bench.rs:157-158) stay on the power-of-two kernels
    for n in (59, 127, 222, 439, 511, 863, 1013, 1700, 3001):
        d = make(fa, n, np.complex64).describe()
        assert "bluestein" in d and "registers" not in d, (n, d)
    for n, want in ((17, "M=36 registers 6x6"), (31, "M=64 registers 8x8"), (191, "M=400 registers 20x20"), (575, "M=1152 registers 36x32")):
        assert want in make(fa, n, np.complex64).describe(), n
    for n, want in ((59, "M=120 registers 12x10"), (127, "M=256 registers 16x16"), (222, "M=480 registers 24x20"), (439, "M=900 registers 30x30"), (511, "M=1024 registers 32x32")):
        assert want in make(fa, n, np.complex128).describe(), n
    # from 2N - 1 > 1152 on: M = R1 x R2 x R3 (a workgroup per transform) where that is at least 1.25 x shorter than the power of two
    for n, dtype, want in ((647, np.complex64, "M=1296 registers 12x12x9"), (722, np.complex128, "M=1600 registers 16x10x10"), (1031, np.complex64, "M=2304 registers 16x12x12"),
                           (1418, np.complex64, "M=3072 registers 16x16x12"), (4097, np.complex128, "M=8820 registers 21x21x20"), (4099, np.complex64, "M=8820 registers 21x21x20")):
        assert want in make(fa, n, dtype).describe(), (n, make(fa, n, dtype).describe())
    assert "registers" not in make(fa, 863, np.complex128).describe() and "registers" not in make(fa, 5003, np.complex128).describe()
    with pytest.raises(fa.FourierError):
        make(fa, 4096, np.complex64).set_option("bluestein_smooth_m", 0)
    with pytest.raises(fa.FourierError):
        make(fa, 44100, np.complex64).set_option("bluestein_smooth_m", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,dtype,tol", [(44100, np.complex64, 2e-6), (100000, np.complex64, 2e-6), (20736, np.complex64, 1e-6), (59049, np.complex64, 1e-6),
                                         (30870, np.complex64, 2e-6),
                                         (44100, np.complex128, 1e-9), (13122, np.complex128, 5e-14), (250000, np.complex128, 1e-9), (31250, np.complex128, 1e-9),
                                         (1000000, np.complex128, 1e-9)])
def test_register_resident_tile_passes_against_the_lds_tile_passes(torch, fa, fa_exp, oracle, monkeypatch, n, dtype, tol):
    """Round 6: the mixed-length tile passes keep a column's transform in registers (kernels_regtile.h: L = R1 x R2, one LDS round trip) where
    the length splits into two factors of at most 32; the LDS kernels of rounds 4 - 5 (kernels_tiled.h) stay for the other lengths (125,
    245, 343, 490, everything compiled at run time) and as the A/B arm of the experiments library (FOURIER_NO_REGTILE).  Both against the
    oracle, every code, in place, a ragged batch, ragged tiles; and against each other."""
    x = np.stack([hash_normal(4100 + b, n) for b in range(3 if n < 500000 else 2)]).astype(dtype)
    reg = make(fa, n, dtype)  # (fa_exp is bound: the experiments library, same kernels)
    monkeypatch.setenv("FOURIER_NO_REGTILE", "1")
    lds = make(fa, n, dtype)
    monkeypatch.delenv("FOURIER_NO_REGTILE")
    assert "mixed tiles" in reg.describe() and reg.describe() == lds.describe(), (reg.describe(), lds.describe())
    for code in range(5):
        ref = oracle.transform_batch(x, code, nthreads=2)
        a, b = gpu_batch(torch, fa, reg, x, code), gpu_batch(torch, fa, lds, x, code)
        assert rel_l2(a, ref) <= tol and rel_l2(b, ref) <= tol, (n, code, rel_l2(a, ref), rel_l2(b, ref))
        assert rel_l2(a, b) <= (4e-7 if dtype == np.complex64 else 2e-15), (n, code, rel_l2(a, b))
        assert np.array_equal(gpu_batch(torch, fa, reg, x, code, inplace=True), a), (n, code)
    if n != 15625:  # (125 x 125: both plans run the LDS kernel)
        assert not np.array_equal(gpu_batch(torch, fa, reg, x, 0), gpu_batch(torch, fa, lds, x, 0))  # two different kernels really ran


@pytest.mark.gpu
def test_plan_option_register_stages_moves_a_2a3b_length_off_the_reference_schedule_on_request(torch, fa, oracle):
    """Round 6 (sessions 66 / 67): by default a 2^a 3^b length runs the reference's own schedule, bit-identical to the CPU restatement; under plan
    option "register_stages" = 1 it takes the register-stage kernel regfft_shapes.h lists for it on request (kernels_regfft.h: the same values
    within rounding, 1.04 ... 1.44 x): every code, in place, a ragged batch; 0 restores the bits; lengths without such a kernel refuse."""
    for n, dtype in ((729, np.complex64), (729, np.complex128), (4608, np.complex64), (2592, np.complex128), (13122, np.complex64), (19683, np.complex64),
                     (9216, np.complex128)):
        shape = regfft_shape(n, dtype, on_request=True)
        assert shape is not None, (n, dtype)
        plan = make(fa, n, dtype)
        base = plan.describe()
        assert "mixed-radix" in base
        batch = 67 if n < 5000 else 9
        x = np.stack([hash_normal(5200 + b, n) for b in range(batch)]).astype(dtype)
        want = {code: gpu_batch(torch, fa, plan, x, code) for code in range(5)}
        assert np.array_equal(want[0][:3], oracle.transform_batch(x[:3], 0)), n
        plan.set_option("register_stages", 1)
        assert plan.describe().startswith(f"stockham registers {shape} one-launch"), plan.describe()
        tol, close = (1e-6, 4e-7) if dtype == np.complex64 else (5e-14, 3e-15)
        for code in range(5):
            got = gpu_batch(torch, fa, plan, x, code)
            assert rel_l2(got[:3], oracle.transform_batch(x[:3], code)) <= tol and rel_l2(got, want[code]) <= close, (n, code, rel_l2(got, want[code]))
            assert np.array_equal(gpu_batch(torch, fa, plan, x, code, inplace=True), got), (n, code)
        assert not np.array_equal(gpu_batch(torch, fa, plan, x, 0), want[0])  # another kernel really ran
        plan.set_option("register_stages", 0)
        assert plan.describe() == base and np.array_equal(gpu_batch(torch, fa, plan, x, 0), want[0]), n
    for n in (1024, 1013, 3 * 4096, 96):  # a power of two, a Bluestein length, 2^a 3^b on tile passes, a 2^a 3^b length the A/B left out
        plan = make(fa, n, np.complex64)
        desc = plan.describe()
        with pytest.raises(fa.FourierError):
            plan.set_option("register_stages", 1)
        assert plan.describe() == desc
    plan = make(fa, 1001, np.complex64)
    plan.set_option("register_stages", 1)
    assert "registers 13x11x7" in plan.describe()
    # library-wide (fourier_hip_set_default_option "register_stages_at_create" / FOURIER_HIP_REGISTER_STAGES=1): for callers that only know create
    prev = fa.get_default_option("register_stages_at_create")
    fa.set_default_option("register_stages_at_create", 1)
    try:
        plan = make(fa, 4608, np.complex64)
        assert plan.describe().startswith("stockham registers 18x16x16 one-launch"), plan.describe()
        x = np.stack([hash_normal(5300 + b, 4608) for b in range(5)]).astype(np.complex64)
        assert rel_l2(gpu_batch(torch, fa, plan, x, 0), oracle.transform_batch(x, 0)) <= 1e-6
        assert "mixed-radix" in make(fa, 96, np.complex64).describe()
    finally:
        fa.set_default_option("register_stages_at_create", prev)
    assert "mixed-radix" in make(fa, 4608, np.complex64).describe()


CHIRPZ_REG3_MENU = [1296, 1440, 1600, 2304, 2560, 3072, 8820, 9261]  # M = R1 x R2 x R3
CHIRPZ_REG_MENU = [36, 49, 64, 81, 100, 120, 144, 168, 196, 225, 256, 288, 324, 360, 400, 441, 480, 525, 576, 625, 675, 729, 784, 840, 900, 960, 1024]


def _bluestein_length(n):  # a prime factor above 13
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n > 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_one_launch_chirpz_on_a_smooth_m_in_registers(torch, fa, oracle, dtype):
    """Round 6 (kernels_chirpz.h): a short Bluestein length runs the whole chirp-z in ONE launch on M = R1 x R2 >= 2N - 1
    (bluesteins.rs:110 asks for no more; the reference takes the next power of two) with both M-point transforms in registers and 64 / R1
    lane groups per one-wave workgroup -- or, from 2N - 1 > 1152 on, on M = R1 x R2 x R3 <= 9261 with a workgroup per transform and three
    register stages each way.  Every kernel of the menu, forced (plan option bluestein_smooth_m = 2), at the longest Bluestein length
    its M reaches: all five codes against the oracle, the f64 truth, in place, a batch that does not fill the last wave, against the
    power-of-two kernels (option 0) -- and the default rule on the reference's own prime bench sizes (fft_bench.rs:158)."""
    menu = CHIRPZ_REG_MENU + ([1152] if dtype == np.complex64 else []) + CHIRPZ_REG3_MENU
    tol = 2e-6 if dtype == np.complex64 else 1e-12  # f64: the ORACLE's unreduced chirp angle (bluesteins.rs:10,31,57)
    for m in menu:
        n = next(v for v in range((m + 1) // 2, 0, -1) if _bluestein_length(v))
        plan, pow2 = make(fa, n, dtype), make(fa, n, dtype)
        plan.set_option("bluestein_smooth_m", 2)
        pow2.set_option("bluestein_smooth_m", 0)
        assert f"bluestein M={min(v for v in menu if v >= 2 * n - 1)} registers" in plan.describe() and "one-launch" in plan.describe(), (n, plan.describe())
        assert "registers" not in pow2.describe() and "M=%d " % (1 << int(np.ceil(np.log2(2 * n - 1)))) in pow2.describe(), pow2.describe()
        batch = 133 if m <= 1152 else 7
        x = np.stack([hash_uniform(5100 + b, n) for b in range(batch)]).astype(dtype)
        truth = torch.fft.fft(torch.from_numpy(x).to(torch.complex128)).numpy()
        for code in range(5):
            a = gpu_batch(torch, fa, plan, x, code)
            assert np.array_equal(gpu_batch(torch, fa, plan, x, code, inplace=True), a), (n, code)
            assert rel_l2(a, gpu_batch(torch, fa, pow2, x, code)) <= (4e-7 if dtype == np.complex64 else 4e-15), (n, code)
            if code in (0, 3):
                ref = oracle.transform_batch(x[:7], code)
                assert rel_l2(a[:7], ref) <= tol, (n, code, rel_l2(a[:7], ref))
        assert rel_l2(gpu_batch(torch, fa, plan, x, 0), truth) <= (4e-7 if dtype == np.complex64 else 4e-15), n
        back = gpu_batch(torch, fa, plan, gpu_batch(torch, fa, plan, x, 0), 1)
        assert rel_l2(back, x) <= (6e-7 if dtype == np.complex64 else 6e-15), n
        d = torch.from_numpy(x).cuda()
        names = [p[0] for p in plan.profile_batch_ptr(d.data_ptr(), torch.empty_like(d).data_ptr(), batch, 0, 0) if p[2] > 0]
        assert names == ["bluestein_one_launch"], names
    with pytest.raises(fa.FourierError):
        make(fa, 400, dtype).set_option("bluestein_smooth_m", 2)  # not a Bluestein length
