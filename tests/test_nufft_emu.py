"""The non-uniform FFT handle (fourier_hip_nufft_*, fourier_amd.Nufft) WITHOUT a GPU: the engine sources compiled against the CPU
emulation (tests/emu), driven through the same C ABI / Python layer as the product -- the cases of tests/nufft_cases.py, which the
`-m gpu` twin tests/test_gpu_nufft.py runs on device buffers, against tests/nufft_truth.py.  Measure, bounds and shapes are stated in
tests/nufft_cases.py.  Here also: the handle's w and L against the model's, the model's quadrature rule against 200 nodes, the create contract of
the C ABI, and the allocation-free property after reserve (through the emulator's allocation counter)."""
import ctypes

import numpy as np
import pytest

import nufft_cases as cases
import nufft_truth as truth

REALS = ["f32", "f64"]
TABLES = [0, 1]


@pytest.fixture(scope="module")
def fa():
    from emu import build_emu
    from fourier_amd import _lib

    prev = _lib._lib
    _lib._lib = build_emu.load()  # route the operator layer to the emulation build
    import fourier_amd

    yield fourier_amd
    _lib._lib = prev
    cases.report("emu")


@pytest.fixture
def be(fa, monkeypatch):
    return cases.HostBackend(fa, monkeypatch)


def test_the_handle_and_the_model_agree_on_widths_and_grid_lengths(fa):
    """describe() names the w and L that tests/nufft_truth.py's model computes, for every eps and size of the cases; and the model's
    quadrature rule -- the handle's host code holds the same rule, reached only through the accuracy cases -- is converged"""
    for real in REALS:
        for eps in cases.EPS[real] + (1e-2, 1e-5, 1e-9, 1e-14, 3e-7):
            for n in cases.SIZES:
                w = truth.width(eps, real)
                assert cases.describe_numbers(fa.Nufft(n, eps, real)) == (w, truth.grid_length(n, w)), (real, eps, n)
    assert [truth.width(e, "f32") for e in cases.EPS["f32"]] == [2, 4, 7, 8]
    assert [truth.width(e, "f64") for e in cases.EPS["f64"]] == [2, 4, 7, 13, 16]
    assert [truth.grid_length(n, 7) for n in cases.SIZES] == [15, 15, 15, 15, 200, 216, 1000, 1024]
    assert truth.grid_length(5, 13) == 27 and truth.grid_length(1, 2) == 4
    for w in range(2, 17):
        for length, n in ((2 * w, 1), (2 * w, w), (200, 100), (216, 101), (1000, 500)):
            k = np.arange(n // 2 + 1)
            a, b = truth.phihat(w, length, k), truth.phihat(w, length, k, 200)
            assert np.max(np.abs(a / b - 1)) <= 1e-15, (w, length)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_signs_and_orders(be, real, table, n):
    eps = cases.TIGHT[real]
    cases.accuracy(be, real, n, eps, cases.points("random37", n, eps, real), table, batch=cases.RB + 1, what="sizes")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("name", cases.POINT_SETS)
def test_point_sets(be, real, table, name):
    for n in cases.sizes_for(name):
        eps = cases.TIGHT[real]
        cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, orders=(0,), what=name)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_widths_through_eps(be, real, table):
    for eps in cases.EPS[real]:
        # (the wraps at both ends under every width: first_cell at n = 3, where every footprint wraps, and test_adjointness; points
        # in ONE cell of a 200-cell grid are not a valid input at every width, tests/nufft_cases.py: 2.7 x 10^(1 - w) at w = 8)
        for n, name in ((101, "random37"), (100, "far"), (3, "first_cell"), (500, "random3000")):
            cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, signs=(-1,), orders=(0,), what=f"eps {eps} {name}")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("batch", [1, cases.RB - 1, cases.RB, cases.RB + 1, 2 * cases.RB + 1])
def test_batches(be, real, batch):
    eps = cases.TIGHT[real]
    for table in TABLES:
        cases.accuracy(be, real, 101, eps, cases.points("ties", 101, eps, real), table, batch=batch, signs=(1,), orders=(1,), what="batches")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_adjointness(be, real, table):
    for eps in cases.EPS[real]:
        for n, name in ((100, "random37"), (101, "last_cell"), (101, "first_cell"), (2, "ties"), (100, "below_pi")):
            cases.adjoint(be, real, n, eps, cases.points(name, n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
def test_the_two_routes_agree(be, real):
    for eps in cases.EPS[real]:
        cases.routes_agree(be, real, 101, eps, cases.points("random37", 101, eps, real))


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_orders_permutation_and_repetition_are_bit_exact(be, real, table):
    for n in (100, 101, 3):
        cases.orders_and_permutation(be, real, n, cases.TIGHT[real], table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_launch_walk(be, real, table):
    eps = cases.TIGHT[real]
    for n, name in ((101, "random37"), (5, "random3000")):  # 3000 points: the interpolation beyond one workgroup
        x = cases.points(name, n, eps, real)
        for batch, items in ((2 * cases.RB + 1, 1), (3 * cases.RB, 2 * truth.grid_length(n, truth.width(eps, real))), (cases.RB + 2, 300)):
            cases.launch_walk(be, real, n, eps, x, table, batch, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("rows", [2, 1])
def test_scratch_walk(be, real, table, rows):
    eps = cases.TIGHT[real]
    for n in (100, 101):
        cases.scratch_walk(be, real, n, eps, cases.points("random37", n, eps, real), table, rows)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_a_nan_stays_in_its_row(be, real, table):
    cases.nan_row(be, real, 101, cases.TIGHT[real], cases.points("random37", 101, cases.TIGHT[real], real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_set_points_again_replaces_the_points(be, real, table):
    cases.second_set_points_replaces(be, real, table)


@pytest.mark.parametrize("real", REALS)
def test_refusals_write_nothing(be, real):
    cases.refusals(be, real)


def test_create_and_the_null_handle(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(L, f"fourier_hip_nufft_{op}_{s}")  # noqa: E731
        for n, eps in ((0, 1e-6), (16, 0.0), (16, -1e-3), (16, float("nan")), (16, float("inf")), (1 << 40, 1e-6)):
            assert not fn("create")(n, eps, -1), (n, eps)
        h = fn("create")(16, 1e-6, -1)
        assert h and fn("modes")(h) == 16 and fn("points")(h) == 0
        assert fn("describe")(h).startswith(b"nufft evaluated: w 7, L 32, ")
        assert fn("set_option")(h, None, 1) == cases.INVALID
        assert fn("set_points")(h, None, 3, None) == cases.INVALID and fn("last_status")(h) == cases.INVALID
        assert fn("set_points")(h, None, 0, None) == 0 and fn("last_status")(h) == 0  # no points: valid
        assert fn("reserve")(h, 3) == 0
        fn("destroy")(h)
    with pytest.raises(ValueError):
        fa.Nufft(0, 1e-6, "f32")
    with pytest.raises(ValueError):
        fa.Nufft(16, 0.0, "f64")
    # eps = 1 and above: the narrowest kernel
    assert cases.describe_numbers(fa.Nufft(16, 1.0, "f32")) == (2, 32)
    assert cases.describe_numbers(fa.Nufft(1, 50.0, "f64")) == (2, 4)


def test_calls_after_reserve_do_not_allocate(be):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(30)
    for n, eps in ((101, 1e-6), (512, 1e-12)):
        for table in TABLES:
            plan = cases.make(be, n, eps, "f64", table)
            x = cases.points("random37", n, eps, "f64")
            cases.set_points(be, plan, x)
            plan.reserve(6)
            c, f = cases.crand(rng, (6, len(x)), "f64"), cases.crand(rng, (6, n), "f64")
            oc, of = np.empty_like(c), np.empty_like(f)
            before = L.fourier_emu_alloc_count()
            for b in (1, 6, 3):
                plan.to_modes_ptr(c.ctypes.data, of.ctypes.data, b)
                plan.to_points_ptr(f.ctypes.data, oc.ctypes.data, b)
            assert L.fourier_emu_alloc_count() == before, (n, table)
