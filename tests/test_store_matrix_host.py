"""CPU: the store matrix (``store_matrix_cases.py``) is what it says it is.  The geometry is ragged in every way the
module lists, as the planner (``pyramid.*``, ``z_shard``, ``_device_retile_ok``) sees it, so a later change to the planner
cannot silently make the matrix aligned; the case list is a pairwise cover; the NumPy expectations of the pyramid, the
histogram and the projections agree with the library's host builds on the ragged volume; and the oracle's float32 and
float64 regimes agree on the sampled planes, so the one-count bound of the stripe filter is meetable."""

import itertools
import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine, pyramid
from aind_smartspim_destripe_amd import projections as pr
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.distributed import z_shard
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import destripe_oracle as orc
from oracle import format_oracle as fo
from tests import store_matrix_cases as sm

ZYX = (sm.Z, sm.H, sm.W)
SCALES = [(2, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 1)]


def _block_z(scale):
    return 4 if scale[0] == 1 else sm.BLOCK_Z


# ---- 1. the geometry ------------------------------------------------------------------------------------------------------
def test_blocks_bricks_and_input_chunks_are_ragged():
    co, ci = sm.OUT_CHUNKS[-3:], sm.IN_CHUNKS[-3:]
    blocks = [(z, min(z + sm.BLOCK_Z, sm.Z)) for z in range(0, sm.Z, sm.BLOCK_Z)]
    assert blocks == [(0, 8), (8, 16), (16, 22)]
    assert blocks[-1][1] % co[0] == 2  # the last block ends half-way through an output z chunk
    assert [z0 % ci[0] for z0, _ in blocks] == [0, 2, 1]  # blocks 2 and 3 start inside an input chunk
    assert (sm.H % co[1], sm.W % co[2]) == (6, 4) and (-(-sm.H // co[1]), -(-sm.W // co[2])) == (3, 4)
    assert (sm.W % co[1], sm.H % co[2]) == (4, 6)  # turned by 90 degrees the remainders swap axes
    assert all(n % c for n, c in zip(ZYX, ci)) and all(a % b and b % a for a, b in zip(co, ci))
    assert sm.H % 2 == 0 and sm.W % 2 == 0  # the march route and the device re-tiling take the plane
    # the device path takes this geometry, for one rank and for both ranks of either split
    src = MiniZarrArray(".", {"shape": (1, 1) + ZYX, "chunks": sm.IN_CHUNKS, "dtype": "<u2", "compressor": None})
    dst = MiniZarrArray(".", {"shape": (1, 1) + ZYX, "chunks": sm.OUT_CHUNKS, "dtype": "<u2", "compressor": None})
    for bz, (z0, z1) in itertools.product((4, 8), [(0, 22), (0, 16), (16, 22), (0, 12), (12, 22)]):
        assert zd._device_retile_ok(src, dst, ZYX, bz, z0, z1), (bz, z0, z1)
    # the deleted chunk lies inside the volume, is cut by its right border, and two z blocks of either size read it
    region = sm.missing_region()
    assert [(s.start, s.stop) for s in region] == [(15, 18), (24, 48), (80, 100)]
    for case in (sm.BY_NAME["01-stripes-fused222-runs"], sm.BY_NAME["02-stripes-rot-fused122"]):
        assert sm.expected_decode_routes(case, (0, sm.Z))[1] == 2


@pytest.mark.parametrize("scale", SCALES, ids=["x".join(map(str, s)) for s in SCALES])
def test_the_planner_accepts_the_geometry_and_plans_it_ragged(scale):
    levels = pyramid.fused_levels(ZYX, sm.OUT_CHUNKS, 3, scale)
    assert [(lv.shape, lv.chunks) for lv in levels] == sm.level_geometry(scale, 3)  # the NumPy statement of the levels
    bz = _block_z(scale)
    pyramid.fused_check_blocks(levels, bz, scale)
    if scale[0] == 1:
        with pytest.raises(ValueError):
            pyramid.fused_check_blocks(levels, 8, scale)  # why those cases run z blocks of 4
    sched = pyramid.fused_schedule(levels, 0, sm.Z, bz, scale)
    assert [b for b, _ in sched] == [(z, min(z + bz, sm.Z)) for z in range(0, sm.Z, bz)]
    for lv in levels:  # every chunk row of every level leaves exactly once
        flushed = [s.row for _, shares in sched for s in shares if s.level == lv.level and s.flush]
        assert flushed == list(range(-(-lv.shape[0] // lv.chunks[0]))), (lv, flushed)
    if scale == (2, 2, 2):
        assert [lv.shape for lv in levels] == [(11, 35, 50), (5, 17, 25)]  # odd extents
        assert levels[1].chunks == (4, 17, 25)  # clamped to the level's shape
        l2 = [[s for s in shares if s.level == 2][0] for _, shares in sched]
        # a level-2 chunk row that block 1 opens and block 2 closes; the short last block gives one plane to row 1
        assert [(s.row, s.offset, s.planes, s.first, s.flush) for s in l2] == [(0, 0, 2, True, False), (0, 2, 2, False, True),
                                                                                (1, 0, 1, True, True)]  # fmt: skip
        l1 = [[s for s in shares if s.level == 1][0] for _, shares in sched]
        assert [(s.row, s.planes, s.flush) for s in l1] == [(0, 4, True), (1, 4, True), (2, 3, True)]
    # two ranks: the split of the fused pass, and the plain one
    fused = [pyramid.fused_z_range(sm.Z, 2, r, sm.OUT_CHUNKS[-3], levels, scale) for r in (0, 1)]
    assert fused == ([(0, 16), (16, 22)] if scale[0] == 2 else [(0, 12), (12, 22)])
    assert [z_shard(sm.Z, 2, r, z_chunk=sm.OUT_CHUNKS[-3]) for r in (0, 1)] == [(0, 12), (12, 22)]
    # the stand-alone pipelined pass takes the output's z chunks as its source
    assert pyramid.pipelined_block_z(sm.OUT_CHUNKS[-3], levels, scale) == 4


def test_rank_ranges_of_the_cases_are_the_planners():
    for case in sm.CASES:
        if case.pyramid == "fused":
            levels = pyramid.fused_levels(ZYX, sm.OUT_CHUNKS, case.n_levels, case.scale)
            want = [pyramid.fused_z_range(sm.Z, case.ranks, r, sm.OUT_CHUNKS[-3], levels, case.scale) for r in range(case.ranks)]
            pyramid.fused_check_blocks(levels, sm.block_z(case), case.scale)
        else:
            want = [z_shard(sm.Z, case.ranks, r, z_chunk=sm.OUT_CHUNKS[-3]) for r in range(case.ranks)]
        assert sm.rank_ranges(case) == want, case.name
    starts = {sm.rank_ranges(c)[1][0] for c in sm.CASES if c.ranks == 2}
    assert starts == {12, 16}  # the second rank starts at a non-zero z; at 16 also inside an input chunk
    assert 16 % sm.IN_CHUNKS[-3] != 0 and 12 % sm.BLOCK_Z != 0  # and at 12 off the seams of z blocks of 8 that start at 0


# ---- 2. the case list -----------------------------------------------------------------------------------------------------
def test_the_cases_are_a_pairwise_cover():
    assert sm.uncovered_pairs() == []
    assert len({c.name for c in sm.CASES}) == len(sm.CASES) <= 18
    dropped = [c for c in sm.CASES if c.name != "09-lightsheet-rot-host-path-zlib"]
    assert ("retile", False, "rotate", True) in sm.uncovered_pairs(dropped)  # the check does see a hole
    entry = [c for c in sm.CASES if c.entry]
    assert len(entry) == 6 and {c.filter for c in entry} == {"stripes", "streaks", "lightsheet"}
    host = sm.BY_NAME["09-lightsheet-rot-host-path-zlib"]  # the host path with rotate + lightsheet + projections
    assert (host.retile, host.rotate, host.filter, host.proj) == (False, True, "lightsheet", "both")
    assert any(c.n_levels == 1 for c in sm.CASES)
    for c in sm.CASES:  # what the options need of each other
        assert c.filter != "lightsheet" or not c.shading
        assert (c.pyramid is None) == (c.scale is None) == (c.n_levels == 1)
        assert c.retile or not (c.codec or c.decode or c.pyramid == "fused")
        assert not c.codec or c.out == "blosc" or c.out == sm.LZ4
        assert sm.codec_mode(c) != "runs" or c.out == "blosc"


# ---- 3. the input ---------------------------------------------------------------------------------------------------------
def test_the_input_has_both_configs_glow_and_a_hole(tmp_path):
    vol, seen = sm.volume(), sm.effective_volume()
    assert vol.shape == ZYX and vol.dtype == np.uint16 and not vol.flags["WRITEABLE"] and not seen.flags["WRITEABLE"]
    which = [orc.select_config(seen[z], sm.NO_CELLS, sm.CELLS, sm.HIGH_INT)[0] for z in range(sm.Z)]
    assert which == [1 if z % 4 == 0 else 0 for z in range(sm.Z)]
    assert sorted({which[z] for z in sm.SAMPLED}) == [0, 1]  # both configs among the sampled planes
    turned = [orc.select_config(np.rot90(seen[z]), sm.NO_CELLS, sm.CELLS, sm.HIGH_INT)[0] for z in range(sm.Z)]
    assert turned == which
    assert not np.array_equal(vol, seen) and (seen[sm.missing_region()] == sm.FILL_VALUE).all()
    tile = sm.write_input(tmp_path, "blosc")
    src = MiniZarrArray.open(os.path.join(tile, "0"))
    assert src.chunks == sm.IN_CHUNKS and src.fill_value == sm.FILL_VALUE
    assert np.array_equal(src[0, 0], seen)  # the host reader fills the hole


# ---- 4. the NumPy expectations against the library's host builds, on the ragged volume -----------------------------------------
@pytest.mark.parametrize("scale", SCALES, ids=["x".join(map(str, s)) for s in SCALES])
def test_numpy_pyramid_is_the_host_build_block_by_block(scale):
    """``dsx_pyramid_block_scale_ref`` fed the z blocks of the store pass by the planner's schedule (offsets inside a
    chunk row, rows that two blocks fill, the short last block) gives the bricks of ``fo.pyramid``."""
    vol = sm.effective_volume()
    case = sm.Case("x", "stripes", None, False, False, "fused", scale, 3, "blosc", False, False, False, "output", 1, True, False)
    want = [sm.expected_bricks(lvl, ck) for lvl, (_, ck) in zip(sm.expected_levels(vol, case), sm.level_geometry(scale, 3))]
    levels = pyramid.fused_levels(ZYX, sm.OUT_CHUNKS, 3, scale)
    chunks = [lv.chunks for lv in levels]
    grid = [(-(-lv.shape[1] // lv.chunks[1]), -(-lv.shape[2] // lv.chunks[2])) for lv in levels]
    cur = [np.zeros((1,) + g + ck, np.uint16) for g, ck in zip(grid, chunks)]
    got = [{} for _ in levels]
    for (z0, z1), shares in pyramid.fused_schedule(levels, 0, sm.Z, _block_z(scale), scale):
        for i, s in enumerate(shares):
            if s.first:
                cur[i][:] = 0
        engine.pyramid_block_ref(vol[z0:z1], chunks, z0s=[s.offset for s in shares], bricks=cur, rows=[1] * len(levels),
                                 scale=scale)  # fmt: skip
        for i, s in enumerate(shares):
            if s.flush:
                for by, bx in itertools.product(*map(range, grid[i])):
                    got[i][(s.row, by, bx)] = cur[i][0, by, bx].copy()
    for i in range(len(levels)):
        assert sorted(got[i]) == sorted(want[i]), (scale, i)
        for idx in want[i]:
            assert np.array_equal(got[i][idx], want[i][idx]), (scale, i, idx)
    # and the whole volume as one block
    whole = engine.pyramid_block_ref(vol, chunks, scale=scale)
    for i in range(len(levels)):
        assert np.array_equal(whole[i], fo.planes_to_bricks(sm.expected_levels(vol, case)[i], chunks[i])), (scale, i)


def test_numpy_histogram_and_projections_are_the_host_builds():
    vol = sm.effective_volume()
    hist = np.zeros(65536, np.int64)
    acc = {name: np.zeros(shape, dtype) for name, shape, dtype in engine.projection_shapes(ZYX)}
    for z0 in range(0, sm.Z, sm.BLOCK_Z):  # blocks of 8, 8 and 6 planes, the projections at a non-zero z_off
        block = vol[z0 : z0 + sm.BLOCK_Z]
        engine.volhist_ref(block, hist)
        engine.project_ref(block, acc=acc, z_off=z0)
    want_hist = sm.expected_histogram(vol)
    assert int(want_hist.sum()) == 22 * 70 * 100 and np.array_equal(hist, want_hist)
    want = pr.project_volume(vol)
    for name in pr.NAMES:
        assert acc[name].dtype == want[name].dtype and np.array_equal(acc[name], want[name]), name
    assert want["max_z"].shape == (sm.H, sm.W) and want["sum_x"].shape == (sm.Z, sm.H) and want["sum_y"].shape == (sm.Z, sm.W)
    assert sm.expected_window(vol) == zd.display_window_from_histogram(want_hist)


# ---- 5. the seed ----------------------------------------------------------------------------------------------------------
def test_oracle_regimes_agree_on_the_sampled_planes():
    """The reference computes in float64 from uint16 planes and in float32 from float32 planes; an Otsu plateau that the
    last bits decide would part the two by far more than a count.  With this seed they agree within one count on every
    sampled plane under every stripe configuration of the matrix, so no sampled plane needs an exemption."""
    seen = sm.effective_volume()
    for rotate, shaded in itertools.product((False, True), repeat=2):
        for z in sm.SAMPLED:
            a = sm.stripes_reference(seen[z], rotate, shaded).astype(np.int64)
            b = sm.stripes_reference(seen[z].astype(np.float32), rotate, shaded).astype(np.int64)
            assert np.abs(a - b).max() <= 1, (rotate, shaded, z, int(np.abs(a - b).max()))
            assert not np.array_equal(a, seen[z])  # the filter changes the plane
    ls = sm.independent_plane(sm.BY_NAME["12-lightsheet-pipelined212"], seen[7])
    assert ls[1] == 0 and (ls[0] != seen[7]).mean() > 0.5  # the light-sheet mode changes pixels
