"""K13 on the MI355X where its loops take more than one trip: vd_pairs_kernel at two rounds of its 1024-workgroup grid,
the row loops of vd_plane_bound_kernel and vd_final_kernel beyond 64 and 256 rows, 17 and 20 chunks of vd_bound_kernel,
ties across rounds and across workgroups. The inputs are volume_diameter_trip_cases (which case turns which loop stands in
its docstring; test_volume_diameter_trip_cases.py asserts those properties on the CPU from the golden model). Everything is
compared with == against the golden model; the records are exact integers. What each test runs that no other test does:
  test_equals_golden_where_the_loops_turn      every case, connectivity and spacing, the tile skipping on and off
  test_t_bar_winner_of_the_second_round        a pair only round 1 compares has to replace round 0's best; a perpendicular
                                               end at y = 290, in the second trip of the final kernel's row loop
  test_two_bars_ties_across_rounds             the axial maximum in plane 0 (round 0) and plane 129 (round 1): plane 0 stays;
                                               the two diagonals from different workgroups: the first one wins
  test_sheets_lesions_of_the_second_round      the lesions whose items lie wholly in round 1 have their records
  test_grids_of_different_sizes_on_one_buffer  1024 workgroups, a tiny volume, 307 workgroups, 1024 at N = 1, 1024 again on
                                               the cached work buffers: the final kernel reads this call's slots only
  test_ring_twice                              no dependence on the order of workgroups where hundreds of tile pairs survive
  test_lesions_op_unchanged_next_to_the_diameters   K10's records before and after K13 on 64 lesions"""
import functools

import numpy as np
import pytest
import torch

from nm03_capstone_project_amd import ops

import volume_diameter_cases as vdc
import volume_diameter_trip_cases as tc
import volume_lesion_cases as vlc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The case's mask on the GPU, shared by the tests (no op writes into it)."""
    return torch.from_numpy(tc.case(name)[0].astype(bool)).cuda()


@functools.lru_cache(maxsize=None)
def _golden(native, name, um, conn):
    mask, n, _ = tc.case(name)
    return native.golden_measure_volume_diameters(mask, n, um, conn)


def _gpu(name, um, conn, **kw):
    return ops.measure_volume_diameters(_dev(name), tc.case(name)[1], um, conn, **kw)


@pytest.mark.parametrize("conn", vdc.CONNS)
@pytest.mark.parametrize("name", [c[0] for c in tc.CASES])
def test_equals_golden_where_the_loops_turn(native, name, conn):
    for um in tc.case(name)[2]:
        golden = _golden(native, name, um, conn)
        assert len(golden) == tc.case(name)[1]
        assert _gpu(name, um, conn) == golden, um
        assert _gpu(name, um, conn, brute_force=True) == golden, um


@pytest.mark.parametrize("conn", vdc.CONNS)
def test_t_bar_winner_of_the_second_round(native, conn):
    for brute in (False, True):
        (iso,) = _gpu("t_bar", tc.ISO, conn, brute_force=brute)
        # (2, 0, 129) - (2, 299, 129) lies in tile pair (302, 304): item 369 656 of 372 100, past the first 262 144
        assert iso["major"] == [2, 0, 129, 2, 299, 129] and iso["major_um2"] == 89_401_000_000, "the winner of round 1 is lost"
        assert iso["axial_z"] == 129 and iso["axial"] == [2, 0, 2, 299] and iso["axial_um2"] == 89_401_000_000
        assert iso["axial_perp"] == [6, 290, 2, 0] and iso["axial_perp_extent"] == 1196, "the row loop's second trip (y >= 256)"
        (aniso,) = _gpu("t_bar", tc.ANISO, conn, brute_force=brute)
        assert aniso["major"] == [2, 150, 0, 2, 0, 129] and aniso["major_um2"] == 204_629_490_000, "round 0's winner did not survive round 1"
        assert aniso["axial_z"] == 129 and aniso["axial"] == [2, 0, 2, 299], "the axial winner of round 1 is lost"
        assert aniso["axial_perp"] == [6, 290, 2, 0] and aniso["axial_perp_extent"] == 1196
        assert [iso] == _golden(native, "t_bar", tc.ISO, conn) and [aniso] == _golden(native, "t_bar", tc.ANISO, conn)


@pytest.mark.parametrize("conn", vdc.CONNS)
def test_two_bars_ties_across_rounds(native, conn):
    for um in tc.case("two_bars")[2]:
        for brute in (False, True):
            (rec,) = _gpu("two_bars", um, conn, brute_force=brute)
            assert rec["axial_um2"] == (299 * um[1]) ** 2
            assert rec["axial_z"] == 0 and rec["axial"] == [2, 0, 2, 299], "the tie between round 0 and round 1 went to the later plane"
            assert rec["major"] == [2, 0, 0, 2, 299, 129], "the tie between two workgroups went to the later diagonal"
            assert rec["major_um2"] == (299 * um[1]) ** 2 + (129 * um[2]) ** 2
            assert [rec] == _golden(native, "two_bars", um, conn)


@pytest.mark.parametrize("conn", vdc.CONNS)
def test_sheets_lesions_of_the_second_round(native, conn):
    for um in tc.case("sheets-64")[2]:
        golden = _golden(native, "sheets-64", um, conn)
        for brute in (False, True):
            got = _gpu("sheets-64", um, conn, brute_force=brute)
            assert len(got) == 64
            for r in tc.SHEETS_LATE_RANKS:  # every item of these lesions lies in round 1
                assert got[r]["major_um2"] > got[r]["axial_um2"] > 0, (r, got[r])
                assert got[r] == golden[r], r
                assert vdc.pair_holds(got[r], um)
            assert got[:56] == golden[:56]  # round 0 and the lesion on the boundary
        assert _gpu("sheets-16", um, conn) == golden[:16]  # the control: one round of 307 workgroups


def test_grids_of_different_sizes_on_one_buffer(native):
    """One process, the cached work buffers: a call's final kernel must read the slots its own grid wrote, whatever a
    larger grid, another N or another volume left there."""
    um, conn = tc.ANISO, 26
    small = vlc.word_straddle(65)
    ts = torch.from_numpy(small.astype(bool)).cuda()
    assert _gpu("sheets-64", um, conn) == _golden(native, "sheets-64", um, conn)    # 1024 workgroups, two rounds, 64 slots each
    assert ops.measure_volume_diameters(ts, 3, um, conn) == native.golden_measure_volume_diameters(small, 3, um, conn)
    assert _gpu("sheets-16", um, conn) == _golden(native, "sheets-16", um, conn)    # 307 workgroups, one round, 16 slots each
    assert _gpu("t_bar", um, conn) == _golden(native, "t_bar", um, conn)            # 1024 workgroups, one slot each
    assert _gpu("sheets-64", um, conn) == _golden(native, "sheets-64", um, conn)


def test_ring_twice(native):
    first = _gpu("ring", tc.CIRCULAR, 26)
    assert first == _gpu("ring", tc.CIRCULAR, 26)
    assert first == _golden(native, "ring", tc.CIRCULAR, 26)
    (rec,) = first
    assert rec["major_um2"] == 28_216_760_000 and rec["major"] == [3, 64, 17, 4, 235, 112]
    assert rec["axial_z"] == 60 and rec["axial_um2"] == 28_023_760_000


def test_lesions_op_unchanged_next_to_the_diameters(native):
    """ops.measure_volume_lesions on the sheets before and after a diameter call of two rounds: the same records, equal
    to golden."""
    mask = tc.sheets()
    region, raw = vlc.inputs(mask)
    t = (_dev("sheets-64"), torch.from_numpy(region.astype(bool)).cuda(), torch.from_numpy(raw.view(np.int16)).cuda())
    before = ops.measure_volume_lesions(*t, 64, 26)
    dia = ops.measure_volume_diameters(t[0], 64, tc.ISO, 26)
    assert ops.measure_volume_lesions(*t, 64, 26) == before
    assert before[1] == native.golden_measure_volume_lesions(mask, raw, 64, "u16", 16, 26)
    assert before[0] == native.golden_measure_volume(mask, region, raw, "u16", 16, 26)
    assert dia == _golden(native, "sheets-64", tc.ISO, 26)
