"""The generated kernel tables are consistent with themselves and with the tests that name their rows (CPU, no library needed): the
register-stage rows of fourier_amd/csrc/regfft_shapes.h (tools/gen_regfft_shapes.py) and the tile-pass menus of kernels_regtile.cpp /
kernels_tiled.cpp.  tests/test_gpu_tables.py runs every one of these kernels on the GPU; this file keeps the tables it walks honest."""
import os
import re

import kernel_tables as kt

HERE = os.path.dirname(os.path.abspath(__file__))


def _emu_test_source():
    with open(os.path.join(HERE, "test_engine_emu.py")) as f:
        return f.read()


def test_every_row_is_parsed():
    rows = kt.regfft_rows()
    assert len(rows) == kt.regfft_row_lines() == 834


def test_register_stage_rows_multiply_out_to_their_length():
    for r in kt.regfft_rows():
        assert r.r1 * r.r2 * (r.r3 or 1) == r.n, r
        # the generator's splits: descending stages of at least 2 points, two stages of at most 32 points, three of at most 40, a stage of
        # R1 x R2 lanes within a 1024-lane workgroup (tools/gen_regfft_shapes.py: split2, split3)
        assert r.r1 >= r.r2 >= 2 and (r.r3 == 0 or r.r2 >= r.r3 >= 2), r
        assert r.r1 <= (40 if r.r3 else 32), r
        assert r.r3 == 0 or r.r1 * r.r2 <= 1024, r
        assert 14 <= r.n <= 20480 and kt.is_smooth(r.n), r


def test_register_stage_lengths_are_unique_and_ascend():
    rows = kt.regfft_rows()
    lengths = [r.n for r in rows]
    assert len(set(lengths)) == len(lengths), sorted(n for n in set(lengths) if lengths.count(n) > 1)
    for kind in (False, True):
        own = [r.n for r in rows if r.on_request == kind]
        assert own == sorted(own), kind
    # the default rows have a prime factor of 5 ... 13; the rows on request are the 2^a 3^b lengths that are no power of two (plan.h: regfft_route)
    for r in rows:
        assert kt.is_smooth(r.n, (2, 3)) == r.on_request, r
        assert r.n & (r.n - 1), r


def test_variant_flags_are_the_documented_ones():
    """0 = not adopted, 1 = adopted; three stages: 2 = split-plane exchanges, 3 = factored twiddle tables, 4 = both; f32 three stages: 5 / 6 =
    one transform per workgroup without / with factored tables.  (9 and 10 + F are A/B builds and never committed.)"""
    for r in kt.regfft_rows():
        assert r.f32 in range(7) and r.f64 in range(5), r
        if r.r3 == 0:
            assert r.f32 in (0, 1) and r.f64 in (0, 1), r
        assert r.emu in (0, 1), r
        assert r.f32 or r.f64, r  # a row nobody adopted is not written


def test_count_lines_of_the_header_agree_with_its_rows():
    rows = kt.regfft_rows()
    default, on_request = kt.regfft_counts()
    for kind, want in ((False, default), (True, on_request)):
        own = [r for r in rows if r.on_request == kind]
        assert (len(own), sum(1 for r in own if r.f32), sum(1 for r in own if r.f64)) == want, kind
    assert default == (791, 736, 763) and on_request[0] == 43


def test_rows_of_the_emulator_build_are_the_ones_its_test_names():
    src = _emu_test_source()
    m = re.search(r"^REGFFT_LENGTHS = \(([\d, ]+)\)", src, re.M)
    named = {int(v) for v in m.group(1).split(",")}
    body = src[src.index("def test_plan_option_register_stages_moves_a_2a3b_length_off_the_reference_schedule_on_request"):]
    named_on_request = {int(v) for v in re.search(r"for n in \(([\d, ]+)\):", body).group(1).split(",")}
    rows = kt.regfft_rows()
    assert {r.n for r in rows if r.emu and not r.on_request} == named
    assert {r.n for r in rows if r.emu and r.on_request} == named_on_request


def test_tile_menus_list_no_length_twice_and_only_lengths_a_tile_can_have():
    short, long_ = kt.regtile_menu()
    lds = kt.lds_tile_menu()
    assert sorted(short) == sorted(long_) == sorted(lds) == [0, 1, 2, 3]
    for menu in ({i: short[i] + long_[i] for i in short}, lds):
        flat = [v for i in sorted(menu) for v in menu[i]]
        assert len(set(flat)) == len(flat), sorted(v for v in set(flat) if flat.count(v) > 1)
        for v in flat:
            assert 64 <= v <= 1024 and kt.is_smooth(v), v
    for i in short:
        assert all(64 <= v <= 512 for v in short[i]) and all(512 < v <= 1024 for v in long_[i]), i
        assert all(kt.is_smooth(v, (2, 3, 5, 7)) for v in short[i] + long_[i]), i  # TiledMixedEngine::handles_smooth: prime factors up to 7
        # a register-tile kernel per length of the LDS kernels' menu, shard by shard (engine_tiled.h: pass_kernel falls back to the LDS kernel
        # of the same length where the register one is an empty record)
        assert short[i] == lds[i], i


def test_tile_cover_table_accounts_for_every_menu_length():
    """tests/golden/table_cover.json and the reasoned lists of tests/test_gpu_tables.py: every tile-menu length, in each precision and role,
    in exactly one of them (the GPU test asserts the table's descriptions against the plans)"""
    import test_gpu_tables

    test_gpu_tables.tile_cover_accounts_for_every_length()
