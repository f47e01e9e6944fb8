"""CPU tests of tests/x3_slot_map.py, the Python statement of the persistent fp16x3 linear's slot -> tile map (csrc/gemm_x3.hip): every
tile of every swept shape is owned by exactly one workgroup, and at a 256-workgroup grid (the MI355X's 256 CUs) the shapes of
tests/test_gpu_x3_variants.py fall into the classes that file relies on."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_slot_map as sm  # noqa: E402

GRIDS = (8, 64, 256, 304)
NS = (128, 256, 384, 1024, 1920, 2048, 3072, 4096)
MS = (1, 255, 256, 257, 1731, 4353, 8449, 16540, 20481, 40000)


@pytest.mark.parametrize("N", NS)
def test_every_tile_is_owned_exactly_once(N):
    for M in MS:
        geo = sm.geometry(M, N)
        assert geo["sup_cols"] * geo["sup_n"] >= geo["tiles_n"] and geo["sup_rows"] * geo["sup_cols"] <= 64 and geo["sup_rows"] >= 1
        want = sorted((tm, tn) for tm in range(geo["tiles_m"]) for tn in range(geo["tiles_n"]))
        for grid in GRIDS:
            g = min(grid, geo["n_slots"])
            streams = sm.plan(M, N, g)
            assert len(streams) == g
            got = sorted(t for s in streams for t in s)
            assert got == want, (M, N, grid)
            # slot % 8 is the XCD and grid % 8 == 0: a workgroup's tiles all belong to super-tiles of one XCD
            for wg, s in enumerate(streams):
                for tm, tn in s:
                    sup = (tm // geo["sup_rows"]) * geo["sup_n"] + tn // geo["sup_cols"]
                    assert sup % 8 == wg % 8


def test_grid_of_the_launcher():
    assert sm.grid_for(256, 1024) == 256 and sm.grid_for(304, 1024) == 304 and sm.grid_for(300, 1024) == 296
    assert sm.grid_for(4, 512) == 8 and sm.grid_for(256, 64) == 64
    assert sm.plan_for_cus(8449, 256, 256) == sm.plan(8449, 256, 256)


@pytest.mark.parametrize("N", [256, 128])
def test_8449_rows_give_two_workgroups_a_second_tile_at_256(N):
    streams = sm.plan(8449, N, 256)
    multi = [s for s in streams if len(s) > 1]
    assert multi == [[(0, 0), (32, 0)], [(1, 0), (33, 0)]]
    assert max(len(s) for s in streams) == 2


def test_4353_by_384_puts_a_half_wide_tile_second_at_256():
    geo = sm.geometry(4353, 384)
    streams = sm.plan(4353, 384, 256)
    assert max(len(s) for s in streams) == 2
    assert any(len(s) == 2 and sm.is_half_wide(s[1], geo) for s in streams)
    assert any(len(s) == 2 and sm.is_half_wide(s[1], geo) and sm.is_ragged_m(s[1], geo) for s in streams)
    assert any(len(s) == 2 and not sm.is_half_wide(s[1], geo) for s in streams)


@pytest.mark.parametrize("N", [2048, 1920])
def test_16540_rows_give_three_tile_streams_with_the_ragged_tile_last_at_256(N):
    geo = sm.geometry(16540, N)
    streams = sm.plan(16540, N, 256)
    three = [s for s in streams if len(s) == 3]
    assert three == [[(0, c), (4, c), (64, c)] for c in range(8)]
    assert all(sm.is_ragged_m(s[2], geo) and not sm.is_ragged_m(s[1], geo) for s in three)
    assert max(len(s) for s in streams) == 3 and min(len(s) for s in streams) == 2
    if N == 1920:
        assert sm.is_half_wide(three[7][1], geo) and sm.is_half_wide(three[7][2], geo)       # a half-wide MIDDLE and last tile


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_find_m_reaches_each_class_on_other_cu_counts(cus):
    """What the GPU test does on a device that is not 256 CUs wide: search M over tiles_m until the plan has the class."""
    for N, depth in ((256, 2), (128, 2), (384, 2), (2048, 3), (1920, 3)):
        M = sm.find_m(N, cus, lambda st, geo, d=depth: max(len(s) for s in st) >= d and any(len(s) >= d and sm.is_ragged_m(s[-1], geo) for s in st))
        assert M is not None and M % 256 == 1, (cus, N)
        st = sm.plan_for_cus(M, N, cus)
        assert max(len(s) for s in st) >= depth
    assert sm.find_m(256, 256, lambda st, geo: max(len(s) for s in st) >= 2) == 256 * 32 + 1
