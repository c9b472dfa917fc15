"""The 3-D non-uniform FFT handle (fourier_hip_nufft3d_*, fourier_amd.Nufft3d) WITHOUT a GPU: the engine sources compiled against the
CPU emulation (tests/emu), driven through the same C ABI / Python layer as the product -- the cases of tests/nufft3d_cases.py, which
the `-m gpu` twin tests/test_gpu_nufft3d.py runs on device buffers, against tests/nufft3d_truth.py.  Measure, bounds and shapes are
stated in tests/nufft3d_cases.py.  Here also: the handle's w and L1 x L2 x L3 against the model's, the create contract of the C ABI,
and the allocation-free property after reserve (through the emulator's allocation counter)."""
import ctypes

import numpy as np
import pytest

import nufft3d_cases as cases
import nufft3d_truth as truth

REALS = ["f32", "f64"]
TABLES = [0, 1]
RB = cases.RB
WALK_SIZES = ((16, 16, 16), (30, 4, 9), (20, 6, 21))


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
    """describe() names the w and L1 x L2 x L3 that the model computes, for every eps and size of the cases"""
    for real in REALS:
        for eps in cases.EPS[real] + (1e-2, 1e-5, 1e-9, 1e-14, 3e-7):
            for n in cases.SIZES:
                assert cases.describe_numbers(fa.Nufft3d(n, eps, real)) == (truth.width(eps, real),) + cases.grid(n, eps, real), (real, eps, n)
    assert cases.grid((8, 9, 10), 1e-6, "f32") == (16, 18, 20) and cases.grid((8, 9, 10), 1e-12, "f64") == (27, 27, 27)
    assert cases.grid((20, 6, 21), 1e-6, "f32") == (40, 15, 45) and cases.grid((30, 4, 9), 1e-6, "f32") == (60, 15, 18)
    assert cases.grid((1, 1, 1), 0.5, "f32") == (4, 4, 4) and cases.grid((16, 16, 16), 1e-12, "f64") == (32, 32, 32)
    assert cases.grid((3, 40, 5), 1e-6, "f32") == (15, 80, 15)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_signs_and_orders(be, real, table, n):
    eps = cases.TIGHT[real]
    cases.accuracy(be, real, n, eps, cases.points("random37", n, eps, real), table, batch=RB + 1, what="sizes")


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
        # (the wraps on all three axes under every width: corner_cell at (2, 3, 4), where L = 2 w on every axis at the wider kernels)
        for n, name in (((8, 9, 10), "random37"), ((3, 40, 5), "far"), ((2, 3, 4), "corner_cell"), ((16, 16, 16), "random3000")):
            cases.accuracy(be, real, n, eps, cases.points(name, n, eps, real), table, batch=2, signs=(-1,), orders=(0,), what=f"eps {eps} {name}")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("batch", [1, RB - 1, RB, RB + 1, 2 * RB + 1])
def test_batches(be, real, batch):
    eps = cases.TIGHT[real]
    for table in TABLES:
        cases.accuracy(be, real, (8, 9, 10), eps, cases.points("ties", (8, 9, 10), eps, real), table, batch=batch, signs=(1,), orders=(1,), what="batches")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_adjointness(be, real, table):
    for eps in cases.EPS[real]:
        for n, name in (((8, 9, 10), "random37"), ((30, 4, 9), "corner_cell"), ((3, 40, 5), "wrap1"), ((2, 3, 4), "ties"), ((20, 6, 21), "wrap3")):
            cases.adjoint(be, real, n, eps, cases.points(name, n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
def test_the_two_routes_agree(be, real):
    for eps in cases.EPS[real]:
        cases.routes_agree(be, real, (8, 9, 10), eps, cases.points("random37", (8, 9, 10), eps, real))


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_orders_permutation_and_repetition_are_bit_exact(be, real, table):
    for n in ((8, 9, 10), (30, 4, 9), (2, 3, 4)):
        cases.orders_and_permutation(be, real, n, cases.TIGHT[real], table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_scaling_by_powers_of_two_is_exact(be, real, table):
    n, eps = (8, 9, 10), cases.TIGHT[real]
    cases.scaling(be, real, n, eps, cases.points("random37", n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_launch_walk(be, real, table):
    eps = cases.TIGHT[real]
    for n, name in (((8, 9, 10), "random37"), ((2, 3, 4), "random3000")):  # 3000 points: the interpolation beyond one workgroup
        x = cases.points(name, n, eps, real)
        cells = int(np.prod(cases.grid(n, eps, real)))
        for batch, items in ((2 * RB + 1, 1), (3 * RB, 2 * cells), (RB + 2, 300)):
            cases.launch_walk(be, real, n, eps, x, table, batch, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("items", [2, 1])
def test_scratch_walk(be, real, table, items):
    eps = cases.TIGHT[real]
    for n in WALK_SIZES:  # f32 grids 32^3, 60 x 15 x 18 (two even lengths) and 40 x 15 x 45 (one: the accuracy bound only)
        cases.scratch_walk(be, real, n, eps, cases.points("random37", n, eps, real), table, items)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_a_nan_stays_in_its_item(be, real, table):
    n, eps = (8, 9, 10), cases.TIGHT[real]
    cases.nan_item(be, real, n, eps, cases.points("random37", n, eps, real), table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_no_result_depends_on_the_handles_history(be, real, table):
    cases.history(be, real, table)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("table", TABLES)
def test_one_mode_on_axis_3_agrees_with_the_2d_handle(be, real, table):
    cases.agrees_with_2d(be, real, table)


@pytest.mark.parametrize("real", REALS)
def test_refusals_write_nothing(be, real):
    cases.refusals(be, real)


def test_create_and_the_null_handle(fa):
    from fourier_amd import _lib

    L = _lib.lib()
    for s in _lib.SUFFIXES:
        fn = lambda op: getattr(L, f"fourier_hip_nufft3d_{op}_{s}")  # noqa: E731
        # no modes on an axis, an eps that is not a positive finite number, items above 2^30 bytes (one axis, a product of two, of
        # three, an overflowing product), a grid item above 2^31 bytes (the modes themselves within 2^30 bytes)
        for n1, n2, n3, eps in ((0, 4, 4, 1e-6), (4, 0, 4, 1e-6), (4, 4, 0, 1e-6), (8, 8, 8, 0.0), (8, 8, 8, -1e-3), (8, 8, 8, float("nan")),
                                (8, 8, 8, float("inf")), (1 << 40, 1, 1, 1e-6), (1, 1 << 40, 1, 1e-6), (1, 1, 1 << 40, 1e-6),
                                (1 << 14, 1 << 14, 1, 1e-6), (1, 1 << 14, 1 << 14, 1e-6), (1 << 9, 1 << 9, 1 << 10, 1e-6),
                                (1 << 22, 1 << 22, 1 << 22, 1e-6), (1 << 33, 1 << 33, 1, 1e-6), (1 << 8, 1 << 9, 1 << 9, 1e-6)):
            assert not fn("create")(n1, n2, n3, eps, -1), (n1, n2, n3, eps)
        h = fn("create")(16, 5, 3, 1e-6, -1)
        assert h and fn("modes1")(h) == 16 and fn("modes2")(h) == 5 and fn("modes3")(h) == 3 and fn("points")(h) == 0
        assert fn("describe")(h).startswith(b"nufft3d evaluated: w 7, L 32 x 15 x 15, ")
        assert fn("set_option")(h, None, 1) == cases.INVALID
        assert fn("set_points")(h, None, None, None, 3, None) == cases.INVALID and fn("last_status")(h) == cases.INVALID
        assert fn("set_points")(h, None, None, None, 0, None) == 0 and fn("last_status")(h) == 0  # no points: valid
        assert fn("reserve")(h, 3) == 0
        fn("destroy")(h)
    with pytest.raises(ValueError):
        fa.Nufft3d((0, 4, 4), 1e-6, "f32")
    with pytest.raises(ValueError):
        fa.Nufft3d((8, 8, 8), 0.0, "f64")
    with pytest.raises(ValueError):
        fa.Nufft3d((8, 8), 1e-6, "f32")
    with pytest.raises(ValueError):
        fa.Nufft3d(16, 1e-6, "f32")
    # eps = 1 and above: the narrowest kernel
    assert cases.describe_numbers(fa.Nufft3d((16, 3, 1), 1.0, "f32")) == (2, 32, 6, 4)
    assert cases.describe_numbers(fa.Nufft3d((1, 1, 1), 50.0, "f64")) == (2, 4, 4, 4)


def test_calls_after_reserve_do_not_allocate(be):
    from fourier_amd import _lib

    L = _lib.lib()
    L.fourier_emu_alloc_count.restype = ctypes.c_uint64
    rng = np.random.default_rng(30)
    for n, eps in (((8, 9, 10), 1e-6), ((16, 16, 16), 1e-12), ((30, 4, 9), 1e-3)):
        for table in TABLES:
            plan = cases.make(be, n, eps, "f64", table)
            x = cases.points("random37", n, eps, "f64")
            cases.set_points(be, plan, x)
            plan.reserve(6)
            ins = cases.inputs(rng, 6, n, len(x[0]), "f64")
            oc, of = np.empty_like(ins[1]), np.empty_like(ins[2])
            before = L.fourier_emu_alloc_count()
            for b in (1, 6, 3):
                plan.to_modes_ptr(ins[1].ctypes.data, of.ctypes.data, b)
                plan.to_points_ptr(ins[2].ctypes.data, oc.ctypes.data, b)
            assert L.fourier_emu_alloc_count() == before, (n, table)
