"""DCT / DST of types II and III (fourier_hip_r2r_*, fourier_amd.R2R) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product, checked against the dense definitions and the
extension restatement of tests/r2r_truth.py.  The `-m gpu` twin is tests/test_gpu_r2r.py."""
import ctypes

import numpy as np
import pytest

from helpers import rel_l2
from r2r_truth import KINDS, NORMS, dense, want

INVALID = 1             # FOURIER_HIP_INVALID_ARGUMENT
SIZES = list(range(1, 65)) + [96, 100, 255, 256, 486, 1000, 1001, 4096]
INVERSE_OF = {"dct2": "dct3", "dct3": "dct2", "dst2": "dst3", "dst3": "dst2"}
NORM_OF_INVERSE = {"backward": "forward", "forward": "backward", "ortho": "ortho"}


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


def run(plan, x, kind, norm, out=None):
    x = np.ascontiguousarray(x)
    out = np.empty_like(x) if out is None else out
    plan.transform_batch_ptr(x.ctypes.data, out.ctypes.data, x.shape[0], KINDS[kind], NORMS[norm])
    return out


def error(got, kind, norm, x):
    idx, y = want(kind, norm, x)
    return rel_l2(got[..., idx], y)


@pytest.mark.parametrize("sizes", [SIZES[i::4] for i in range(4)], ids=["a", "b", "c", "d"])
def test_every_kind_and_norm_matches_the_definition(fa, sizes):
    """rel-L2 <= 1e-12: the bound of test_real_emu.py for the same pipeline; the added twiddle c_k is one more f64 rounding."""
    rng = np.random.default_rng(7)
    for n in sizes:
        plan = fa.create_r2r_f64(n)
        x = rng.standard_normal((3, n))
        for kind in KINDS:
            for norm in NORMS:
                err = error(run(plan, x, kind, norm), kind, norm, x)
                assert err <= 1e-12, (n, kind, norm, err)


def test_f32_plans_match_the_definition(fa):
    rng = np.random.default_rng(8)
    for n in (1, 2, 6, 7, 16, 30, 64, 100, 1001, 4096):
        plan = fa.create_r2r_f32(n)
        x = rng.standard_normal((3, n)).astype(np.float32)
        for kind in KINDS:
            for norm in ("backward", "ortho"):
                err = error(run(plan, x, kind, norm), kind, norm, x)
                assert err <= 4e-6, (n, kind, norm, err)


def test_the_truth_agrees_with_scipy_where_scipy_is_installed():
    try:
        import scipy.fft as sf
    except ImportError:
        return
    rng = np.random.default_rng(9)
    for n in (1, 2, 9, 64, 255, 486, 1001):
        x = rng.standard_normal((2, n))
        for kind in KINDS:
            for norm in NORMS:
                ref = (sf.dct if kind.startswith("dct") else sf.dst)(x, type=int(kind[-1]), norm=norm, axis=-1)
                idx, y = want(kind, norm, x)
                assert rel_l2(y, ref[..., idx]) <= 1e-13, (n, kind, norm)


def test_round_trip_returns_the_input(fa):
    rng = np.random.default_rng(10)
    for n in (1, 2, 3, 8, 33, 64, 486, 1001, 4096):
        plan = fa.create_r2r_f64(n)
        x = rng.standard_normal((3, n))
        for kind in KINDS:
            for norm in NORMS:
                back = run(plan, run(plan, x, kind, norm), INVERSE_OF[kind], NORM_OF_INVERSE[norm])
                assert np.allclose(back, x, rtol=0, atol=1e-12), (n, kind, norm)


def test_ortho_matrices_are_orthogonal(fa):
    for n in (8, 9):
        plan = fa.create_r2r_f64(n)
        for kind in KINDS:
            t = run(plan, np.eye(n), kind, "ortho").T  # row b of the output is T e_b: column b of T
            assert np.abs(t @ t.T - np.eye(n)).max() <= 1e-14, (n, kind)
            assert np.abs(t - run(plan, np.eye(n), INVERSE_OF[kind], "ortho")).max() <= 1e-14, (n, kind)  # T^-1 = T^t


def test_in_place_equals_out_of_place_bit_for_bit_and_the_input_stays(fa):
    rng = np.random.default_rng(11)
    for n in (1, 2, 6, 7, 64, 1000, 1001):
        plan = fa.create_r2r_f64(n)
        x = rng.standard_normal((5, n))
        for kind in KINDS:
            for norm in ("backward", "ortho"):
                before = x.tobytes()
                y = run(plan, x, kind, norm)
                assert x.tobytes() == before, (n, kind)
                z = x.copy()
                run(plan, z, kind, norm, out=z)
                assert z.tobytes() == y.tobytes(), (n, kind, norm)


def test_describe_names_the_path_and_the_inner_plan(fa):
    for n in (2, 64, 100, 4096):
        assert fa.create_r2r_f64(n).describe() == "r2r half-length: " + fa.create_fft_f64(n // 2).describe()
        assert fa.create_r2r_f32(n).describe() == "r2r half-length: " + fa.create_fft_f32(n // 2).describe()
    for n in (1, 15, 1001):
        assert fa.create_r2r_f64(n).describe() == "r2r full-length: " + fa.create_fft_f64(n).describe()
    assert fa.create_r2r_f64(100).size() == 100


def test_invalid_arguments(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    assert not L.fourier_hip_r2r_create_float(0, -1) and not L.fourier_hip_r2r_create_double(0, -1)
    with pytest.raises(fa.FourierError):
        fa.create_r2r_f32(0)
    assert L.fourier_hip_r2r_size_double(None) == 0
    assert L.fourier_hip_r2r_describe_double(None) == b""
    assert L.fourier_hip_r2r_last_status_double(None) == INVALID
    assert L.fourier_hip_r2r_transform_batch_double(None, 16, 16, 1, 0, 0, None) == INVALID
    assert L.fourier_hip_r2r_reserve_double(None, 1) == INVALID
    L.fourier_hip_r2r_destroy_double(None)

    n = 16
    plan = fa.create_r2r_f64(n)
    h = plan._h
    x = np.zeros((2, n))
    y = np.zeros((2, n))
    big = np.zeros(4 * n + 8)
    tr = L.fourier_hip_r2r_transform_batch_double
    for kind in (-1, 4, 100):
        assert tr(h, x.ctypes.data, y.ctypes.data, 2, kind, 0, None) == INVALID
    for norm in (-1, 3):
        assert tr(h, x.ctypes.data, y.ctypes.data, 2, 0, norm, None) == INVALID
    assert L.fourier_hip_r2r_last_status_double(h) == INVALID
    assert tr(h, x.ctypes.data, y.ctypes.data, 2, 0, 0, None) == 0
    assert L.fourier_hip_r2r_last_status_double(h) == 0  # reset on entry
    assert tr(h, big.ctypes.data, big.ctypes.data, 2, 0, 0, None) == 0                    # exactly in place
    assert tr(h, big.ctypes.data, big.ctypes.data + 8 * 16, 2, 0, 0, None) == INVALID     # partial overlap
    assert tr(h, big.ctypes.data + 8 * 16, big.ctypes.data, 2, 3, 1, None) == INVALID
    assert tr(h, big.ctypes.data + 8, y.ctypes.data, 1, 0, 0, None) == INVALID            # 8-byte aligned, 16 needed
    assert tr(h, x.ctypes.data, big.ctypes.data + 8, 1, 0, 0, None) == INVALID
    assert tr(h, None, y.ctypes.data, 1, 0, 0, None) == INVALID
    assert tr(h, x.ctypes.data, None, 1, 0, 0, None) == INVALID
    assert tr(h, x.ctypes.data, y.ctypes.data, 0, 0, 0, None) == 0                        # batch 0: no-op
    with pytest.raises(fa.FourierError):
        plan.transform_batch_ptr(x.ctypes.data, y.ctypes.data, 2, 7, 0)
    f32 = fa.create_r2r_f32(n)
    xf = np.zeros(2 * n + 2, np.float32)
    yf = np.zeros(n, np.float32)
    assert L.fourier_hip_r2r_transform_batch_float(f32._h, xf.ctypes.data + 4, yf.ctypes.data, 1, 0, 0, None) == INVALID
    assert L.fourier_hip_r2r_transform_batch_float(f32._h, xf.ctypes.data + 8, yf.ctypes.data, 1, 0, 0, None) == 0


def test_calls_after_reserve_do_not_allocate(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(12)
    for n in (8, 64, 255, 1000, 1001, 4096):
        plan = fa.create_r2r_f64(n)
        plan.reserve(5)
        x = rng.standard_normal((5, n))
        before = L.fourier_emu_alloc_count()
        for b in (1, 5, 3):
            for kind in KINDS:
                run(plan, x[:b], kind, "backward")
                z = x[:b].copy()
                run(plan, z, kind, "ortho", out=z)
        assert L.fourier_emu_alloc_count() == before, n


def test_batches_larger_than_one_scratch_chunk(fa, monkeypatch):
    rng = np.random.default_rng(13)
    for n in (16, 15, 6, 2, 1):
        per = (2 * (n // 2) if n % 2 == 0 else n) * 16  # even N: both halves of the scratch
        monkeypatch.setenv("FOURIER_REAL_SCRATCH_BYTES", str(2 * per))  # two rows per chunk: a batch of 7 in four chunks
        plan = fa.create_r2r_f64(n)
        monkeypatch.delenv("FOURIER_REAL_SCRATCH_BYTES")
        x = rng.standard_normal((7, n))
        for kind in KINDS:
            for norm in NORMS:
                err = error(run(plan, x, kind, norm), kind, norm, x)
                assert err <= 1e-12, (n, kind, norm, err)
            z = x.copy()
            run(plan, z, kind, "backward", out=z)
            assert z.tobytes() == run(plan, x, kind, "backward").tobytes(), (n, kind)


def test_dense_truth_is_scipys_definition_at_a_hand_checked_point():
    """DCT-II of (1, 0) is (2 cos 0, 2 cos(pi/4)); DST-II of (1, 0) is (2 sin(pi/4), 2 sin(pi/2))."""
    assert np.allclose(dense("dct2", 2) @ [1.0, 0.0], [2.0, np.sqrt(2.0)])
    assert np.allclose(dense("dst2", 2) @ [1.0, 0.0], [np.sqrt(2.0), 2.0])
    assert np.allclose(dense("dct3", 2) @ dense("dct2", 2), 4 * np.eye(2))
    assert np.allclose(dense("dst3", 2) @ dense("dst2", 2), 4 * np.eye(2))
