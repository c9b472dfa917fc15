"""The strided-axis sweep of tests/axis_cases.py WITHOUT a GPU: the subset the CPU emulation build holds, through the same C ABI / Python
layer as the product.  The subset, stated here and not found by probing: every lane case (all 32 axis_lane_kernel lengths in both
precisions), the column-tile cases of N = 64, 256 and 1024 (the tile-pass lengths of the emulation build), every small transpose case.
The `-m gpu` twin, with every column-tile length, the large cases and the N-D cases, is tests/test_gpu_axis_sweep.py."""
import numpy as np
import pytest

import axis_cases as ac


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev


@pytest.fixture
def api(fa):
    return ac.HostApi(fa)


def test_the_case_tables_say_what_they_claim():
    assert sorted(n for part in range(ac.LANE_PARTS) for n in ac.lane_lengths(part)) == list(range(1, 33))
    assert set(ac.COLUMN_N_EMU) <= set(ac.COLUMN_N) == {64, 128, 256, 512, 1024, 2048}
    seen = ac.transpose_residues()
    for what in ("rows", "cols"):
        for residue in (0, 1, 2, 31):
            for blocks in (1, 3):
                assert (what, residue, blocks) in seen, (what, residue, blocks)
    assert 20 <= len(ac.TRANSPOSE_CASES) <= 30 and len(set(ac.TRANSPOSE_CASES)) == len(ac.TRANSPOSE_CASES)
    assert sorted(c for part in range(ac.TRANSPOSE_PARTS) for c in ac.TRANSPOSE_CASES[part::ac.TRANSPOSE_PARTS]) == sorted(ac.TRANSPOSE_CASES)


def test_the_long_double_truth_is_a_dft():
    """the matrix against numpy at lengths where both are far below the bounds it is used for, and its defining properties"""
    rng = np.random.default_rng(1)
    for n in (1, 2, 19, 32, 64):
        x = rng.standard_normal((2, n, 3)) + 1j * rng.standard_normal((2, n, 3))
        for code in ac.CODES:
            assert ac.rel_l2(ac.truth_ld(x, code), ac.truth_np(x, code)) <= 1e-15, (n, code)
        w = ac.dft_matrix(n)
        assert np.abs(w @ np.conj(w).T - n * np.eye(n)).max() <= n * 1e-18  # unitary up to N, in long double
        assert np.all(w[0] == 1) and np.all(w[:, 0] == 1)


def test_the_large_cases_split_as_axis_plan_h_says():
    """the launch splits the GPU twin's large cases claim, derived from the constants of axis_plan.h (no GPU needed to state them)"""
    assert ac.transpose_walk(4096, 32800, 8) == [(32768, [4096]), (32, [4096])]
    assert ac.transpose_walk(4096, 65600, 8) == [(32768, [4092, 4]), (32768, [4092, 4]), (64, [4093, 3])]
    assert ac.transpose_walk(4096, 7, 8) is None
    assert ac.lane_walk((1 << 30) + 96, 1) == [(1, 1 << 30), (1, 96)]
    assert ac.lane_walk(1000003, 1074) == [(1073, 1000003), (1, 1000003)]
    assert ac.lane_walk(300, 5) == [(5, 300)]


@pytest.mark.parametrize("part", range(ac.LANE_PARTS))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_lane_kernels(api, real, part):
    assert ac.lane_cases(api, real, part).calls == 8 * len(ac.LANE_SHAPES) * 5


@pytest.mark.parametrize("which", range(3), ids=["narrowest", "twice", "4096"])
@pytest.mark.parametrize("n", ac.COLUMN_N_EMU)
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_column_tile(api, real, n, which):
    assert ac.column_cases(api, real, n, which).calls > 0


@pytest.mark.parametrize("part", range(ac.TRANSPOSE_PARTS))
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_transpose_route_bit_for_bit(api, real, part):
    assert ac.transpose_cases(api, real, part).calls == 5 * 5
