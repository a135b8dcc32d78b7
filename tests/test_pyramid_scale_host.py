"""The pyramid with a scale factor of 1 or 2 per axis, without a GPU: the two host builds
(``engine.pyramid_block_ref`` / ``pyramid_bricks_ref`` with ``scale``) against the NumPy oracle, the planners of the
fused and the pipelined route, ``_check_scale``, the refusals that precede every file, the OME scales, and the geometry
header built with g++ from ``tests/host/pyramid_scale_check.cpp`` under ASan / UBSan as its own process."""

import inspect
import os
import subprocess

import numpy as np
import pytest

import pyramid_scale_cases as pc
from aind_smartspim_destripe_amd import engine, pyramid, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.distributed import z_shard
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import format_oracle as fo

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = pytest.mark.parametrize("scale", pc.SCALES, ids=pc.scale_id)


@SCALES
@pytest.mark.parametrize("zyx", pc.BLOCKS)
def test_host_builds_equal_the_oracle(scale, zyx):
    """Both host builds, ``n_levels`` 2 to 4, three chunk bases, chunks of a volume the block is all of (clamped) and of
    a taller one; the brick source is poisoned wherever a brick sticks out of the block."""
    vol = pc.block_volume(zyx)
    sources = [(sc, pc.source_bricks(vol, sc)) for sc in ((4, 8, 8), (3, 5, 7))]
    seen = set()
    for n_levels in (2, 3, 4):
        for base in pc.BASES:
            for vol_z in (None, 4096):
                chunks = pc.level_chunks(zyx, base, n_levels, scale, vol_z)
                if not chunks or tuple(chunks) in seen:
                    continue
                seen.add(tuple(chunks))
                n = len(chunks)
                got = engine.pyramid_block_ref(vol, chunks, scale=scale)
                want = pc.expected_bricks(vol, chunks, [0] * n, [g.shape[0] for g in got], scale)
                for lvl, (g, w) in enumerate(zip(got, want), start=1):
                    assert g.shape == w.shape and np.array_equal(g, w), (zyx, scale, base, n_levels, lvl)
                for sc, bricks in sources:
                    again = engine.pyramid_bricks_ref(bricks, zyx, sc, chunks, scale=scale)
                    for lvl, (g, w) in enumerate(zip(again, want), start=1):
                        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (zyx, scale, sc, base, n_levels, lvl)
    assert seen


@SCALES
@pytest.mark.parametrize("zyx", [(8, 20, 44), (7, 9, 11)])
def test_host_builds_at_z_offsets_with_several_rows_and_a_second_block(scale, zyx):
    """The share lands at a non-zero plane of rows that hold more than it; the rest stays 0 in a fresh row, and a second
    block written behind the first leaves the first block's share as it was."""
    vol, vol2 = pc.block_volume(zyx), pc.block_volume(zyx, seed=7)
    chunks = [(5, 4, 16), (3, 3, 5)]
    chunks = chunks[: len(pc.level_chunks(zyx, (64, 128, 128), 3, scale))]
    n = len(chunks)
    share = [pc.extents(zyx, l, scale)[0] for l in range(1, n + 1)]
    z0s = [3, 2][:n]
    z1s = [z + s for z, s in zip(z0s, share)]
    rows = [-(-(z + s) // c[0]) + 1 for z, s, c in zip(z1s, share, chunks)]
    assert all(r > 1 for r in rows)
    want = pc.expected_bricks(vol, chunks, z0s, rows, scale)
    want2 = pc.expected_bricks(vol2, chunks, z1s, rows, scale)
    for build in ("block", "bricks"):
        if build == "block":
            got = engine.pyramid_block_ref(vol, chunks, z0s=z0s, rows=rows, scale=scale)
        else:
            got = engine.pyramid_bricks_ref(pc.source_bricks(vol, (3, 5, 7)), zyx, (3, 5, 7), chunks, z0s=z0s, rows=rows,
                                            scale=scale)  # fmt: skip
        for lvl, (g, w) in enumerate(zip(got, want), start=1):
            assert np.array_equal(g, w), (build, zyx, scale, lvl)
        if build == "block":
            engine.pyramid_block_ref(vol2, chunks, z0s=z1s, bricks=got, rows=rows, scale=scale)
        else:
            engine.pyramid_bricks_ref(pc.source_bricks(vol2, (3, 5, 7)), zyx, (3, 5, 7), chunks, z0s=z1s, bricks_out=got,
                                      rows=rows, scale=scale)  # fmt: skip
        for lvl, (g, w, w2) in enumerate(zip(got, want, want2), start=1):
            assert np.array_equal(g, w | w2), (build, zyx, scale, lvl)  # disjoint planes: the union of both shares


def test_host_builds_refuse_what_the_kernels_do_not_take():
    vol = np.zeros((8, 8, 8), np.uint16)
    for bad in ((1, 1, 1), (2, 2, 4), (3, 2, 2), (0, 2, 2), (2, 2), (1.5, 2, 2)):
        with pytest.raises(ValueError, match="only scale factors"):
            engine.pyramid_block_ref(vol, [(4, 4, 4)], scale=bad)
        with pytest.raises(ValueError, match="only scale factors"):
            engine.pyramid_work_bytes((8, 8, 8), 3, bad)
    with pytest.raises(ValueError):  # z is not reduced: 8 planes from plane 2 need 3 rows of 4
        engine.pyramid_block_ref(vol, [(4, 4, 4)], z0s=[2], rows=[2], scale=(1, 2, 2))
    lib = engine.load_library()
    n = engine.ctypes.c_size_t(0)
    assert lib.dsx_pyramid_work_bytes_scale(8, 8, 8, 1, 1, 1, 3, engine.ctypes.byref(n)) == -1
    # the work buffer: dense levels 1 .. n_levels - 2, each padded to 16 bytes; (2, 2, 2) keeps levels 2 .. n_levels - 2
    assert engine.pyramid_work_bytes((8, 10, 12), 2, (1, 2, 2)) == 0
    assert engine.pyramid_work_bytes((8, 10, 12), 3, (1, 2, 2)) == 8 * 5 * 6 * 2
    assert engine.pyramid_work_bytes((8, 10, 12), 4, (1, 2, 2)) == 8 * 5 * 6 * 2 + (8 * 2 * 3 * 2)
    assert engine.pyramid_work_bytes((7, 9, 11), 3, (2, 1, 2)) == (3 * 9 * 5 * 2 + 15) // 16 * 16
    assert engine.pyramid_work_bytes((8, 10, 12), 3) == 0 == engine.pyramid_work_bytes((8, 10, 12), 3, (2, 2, 2))
    assert engine.pyramid_work_bytes((64, 36, 50), 5, (2, 2, 2)) == engine.pyramid_work_bytes((64, 36, 50), 5) > 0


@SCALES
@pytest.mark.parametrize("Z,H,W,block_z,L", [(150, 36, 50, 64, 3), (131, 20, 44, 8, 4), (70, 10, 12, 16, 4)])
def test_levels_assembled_from_blocks_equal_the_whole_volume_pyramid(scale, Z, H, W, block_z, L):
    """A volume cut by ``fused_schedule``: a short last block, and a ``Z`` that is no multiple of the window."""
    vol = pc.block_volume((Z, H, W))
    levels = pyramid.fused_levels((Z, H, W), (1, 1, 64, 128, 128), L, scale)
    whole = fo.pyramid(vol, L, scale)
    assert [lv.shape for lv in levels] == [w.shape for w in whole[1 : len(levels) + 1]] and len(levels) == L - 1
    pyramid.fused_check_blocks(levels, block_z, scale)
    rows = [-(-lv.shape[0] // lv.chunks[0]) for lv in levels]
    bricks, blocks = None, 0
    for (z0, z1), shares in pyramid.fused_schedule(levels, 0, Z, block_z, scale):
        z0s = [s.row * lv.chunks[0] + s.offset for s, lv in zip(shares, levels)]
        bricks = engine.pyramid_block_ref(vol[z0:z1], [lv.chunks for lv in levels], z0s=z0s, bricks=bricks, rows=rows,
                                          scale=scale)  # fmt: skip
        blocks += 1
    assert blocks == -(-Z // block_z) and Z % block_z
    for lv, b in zip(levels, bricks):
        assert np.array_equal(fo.bricks_to_planes(b, lv.shape), whole[lv.level]), (scale, lv)


def test_every_chunk_row_of_every_level_has_one_owner_when_z_is_not_reduced():
    """``fz == 1``: shards align to the plain output z chunk and every chunk row of every level covers ``cz`` level-0
    planes, so every block of ``cz`` planes opens and flushes one row per level."""
    for scale in ((1, 2, 2), (1, 1, 2)):
        levels = pyramid.fused_levels((1000, 2048, 2048), (1, 1, 64, 128, 128), 4, scale)
        assert [lv.shape[0] for lv in levels] == [1000] * 3 and [lv.chunks[0] for lv in levels] == [64] * 3
        assert pyramid.fused_z_chunk(64, levels, scale=scale) == 64
        assert pyramid.pipelined_block_z(64, levels, scale) == 64 and pyramid.pipelined_block_z(32, levels, scale) == 32
        with pytest.raises(ValueError):
            pyramid.pipelined_block_z(128, levels, scale)  # a block of two chunk rows
        edge = 0
        for rank in range(3):
            z0, z1 = pyramid.fused_z_range(1000, 3, rank, 64, levels, scale)
            assert (z0, z1) == z_shard(1000, 3, rank, z_chunk=64) and z0 == edge
            edge = z1
            for (b0, b1), shares in pyramid.fused_schedule(levels, z0, z1, 64, scale):
                assert [(s.row, s.offset, s.planes, s.first, s.flush) for s in shares] == [(b0 // 64, 0, b1 - b0, True, True)] * 3
        assert edge == 1000
    # z alone is reduced: the windows and chunk rows of (2, 2, 2)
    a = pyramid.fused_levels((192, 2048, 2048), (1, 1, 64, 128, 128), 3, (2, 1, 1))
    b = pyramid.fused_levels((192, 2048, 2048), (1, 1, 64, 128, 128), 3)
    assert [lv.shape for lv in a] == [(96, 2048, 2048), (48, 2048, 2048)]
    assert pyramid.fused_z_chunk(64, a, (2, 1, 1)) == 256
    strip = lambda sched: [(z, [tuple(s) for s in shares]) for z, shares in sched]  # noqa: E731
    assert strip(pyramid.fused_schedule(a, 0, 192, 64, (2, 1, 1))) == strip(pyramid.fused_schedule(b, 0, 192, 64))
    with pytest.raises(ValueError, match="multiple of 4 planes \\(2 x 1 x 1 windows of 2 levels\\)"):
        pyramid.fused_check_blocks(a, 66, (2, 1, 1))


def test_the_default_scale_returns_what_the_helpers_returned_before():
    """The shift arithmetic of the 2 x 2 x 2 planners, restated: the generalised helpers with and without ``scale``."""
    for zyx, chunks, L, block_z, src_cz in [((4096, 2048, 2048), (1, 1, 64, 128, 128), 3, 64, 64), ((96, 1600, 2000), (1, 1, 64, 128, 128), 4, 64, 32),
                                            ((70, 10, 12), (64, 128, 128), 5, 16, 8), ((16, 64, 96), (1, 1, 4, 32, 32), 3, 4, 2),
                                            ((3, 2, 2), (64, 128, 128), 4, 2, 1), ((131, 20, 44), (8, 8, 8), 4, 8, 8)]:  # fmt: skip
        cur, want = tuple(zyx), []
        for i in range(1, L):
            if min(cur) < 2:
                break
            cur = tuple(n // 2 for n in cur)
            want.append(pyramid.FusedLevel(i, cur, tuple(min(c, n) for c, n in zip(chunks[-3:], cur))))
        for kw in ({}, {"scale": (2, 2, 2)}):
            levels = pyramid.fused_levels(zyx, chunks, L, **kw)
            assert levels == want and all(type(v) is int for lv in levels for v in lv.shape + lv.chunks)
            zc = pyramid.fused_z_chunk(chunks[-3], levels, **kw)
            assert zc == chunks[-3] << len(levels) and type(zc) is int
            for world, rank in ((1, 0), (3, 1), (8, 7)):
                assert pyramid.fused_z_range(zyx[0], world, rank, chunks[-3], levels, **kw) == z_shard(zyx[0], world, rank, z_chunk=zc)
            pyramid.fused_check_blocks(levels, block_z, **kw)
            sched = pyramid.fused_schedule(levels, 0, zyx[0], block_z, **kw)
            starts = list(range(0, zyx[0], block_z))
            assert [z for z, _ in sched] == [(z0, min(z0 + block_z, zyx[0])) for z0 in starts]
            for (z0, z1), shares in sched:
                for s, lv in zip(shares, levels):
                    assert tuple(s)[:4] == (lv.level,) + divmod(z0 >> lv.level, lv.chunks[0]) + ((z1 - z0) >> lv.level,)
            assert pyramid.pipelined_block_z(src_cz, levels, **kw) == pyramid.pipelined_block_z(src_cz, levels)
    lv = pyramid.fused_levels((192, 2048, 2048), (1, 1, 64, 128, 128), 3)
    assert pyramid.fused_z_chunk(64, lv) == 256 and pyramid.fused_z_chunk(64, lv, scale=(1, 2, 2)) == 64
    with pytest.raises(ValueError, match="fused_pyramid needs z blocks of a multiple of 4 planes \\(2 x 2 x 2 windows of 2 levels\\), not 66"):
        pyramid.fused_check_blocks(lv, 66)
    for fn in (pyramid.fused_levels, pyramid.fused_z_chunk, pyramid.fused_z_range, pyramid.fused_check_blocks,
               pyramid.fused_schedule, pyramid.pipelined_block_z, engine.pyramid_block_ref, engine.pyramid_bricks_ref,
               engine.pyramid_level_elems, engine.pyramid_work_bytes, engine.DestripeEngine.pyramid_block,
               engine.DestripeEngine.pyramid_bricks, engine.DestripeEngine.downsample2):  # fmt: skip
        assert inspect.signature(fn).parameters["scale"].default == (2, 2, 2), fn


def test_check_scale():
    for scale in pc.SCALES:
        for lead in ((), (1,), (1, 1)):
            assert pyramid._check_scale(lead + scale) == scale
            assert pyramid._check_scale(list(lead + scale)) == scale
        assert pyramid.check_scale_factor(list(scale)) == scale
    assert pyramid._check_scale(np.array([1, 1, 1, 2, 2])) == (1, 2, 2)
    for bad in ((1, 1, 1), (1, 1, 1, 1, 1), (2, 2, 4), (1, 1, 2, 2, 4), (3, 2, 2), (0, 2, 2), 1.5, (1.5, 2, 2), (2, 2),
                (2, 1, 2, 2, 2), (1, 2, 1, 2, 2), ("a", 2, 2), None):  # fmt: skip
        with pytest.raises(ValueError, match="^only scale factors"):
            pyramid._check_scale(bad)
    for bad in ((1, 1, 1), (2, 2, 4), 1.5, (2, 2), (1, 1, 1, 2, 2), None):
        with pytest.raises(ValueError, match="^only scale factors"):
            pyramid.check_scale_factor(bad)


def test_compute_pyramid_reduces_y_and_x_alike():
    """The in-memory entry point keeps refusing a window that treats y and x differently, before a device is touched
    (the pixel of a plane is square); a scale it takes gets as far as the engine."""
    vol = np.zeros((4, 4, 4), np.uint16)
    for fn in (pyramid.compute_pyramid, zd.compute_pyramid):
        for bad in ((2, 2, 1), (1, 2, 1), (1, 1, 2), (2, 1, 2), (1, 1, 2, 2, 1)):
            with pytest.raises(ValueError, match="^only scale factors"):
                fn(vol, 2, bad)
        for bad in ((1, 1, 1), (2, 2, 4), 1.5):
            with pytest.raises(ValueError, match="^only scale factors"):
                fn(vol, 2, bad)
    if engine.load_library().dsx_device_count() == 0:
        for good in ((1, 2, 2), (2, 1, 1), (2, 2, 2), (1, 1, 1, 2, 2)):
            with pytest.raises(engine.DsxError):  # (no device here: the argument checks have passed)
                pyramid.compute_pyramid(vol, 2, good)


def _level0(tmp_path, Z=8, H=16, W=16, chunks=(1, 1, 2, 8, 8)):
    p = str(tmp_path / "in.zarr")
    src = MiniZarrArray.create(p, (1, 1, Z, H, W), chunks, np.uint16)
    src[0, 0] = np.arange(Z * H * W, dtype=np.uint16).reshape(Z, H, W)
    return p


@pytest.mark.parametrize("bad", [(1, 1, 1), (2, 2, 4), (3, 2, 2), 1.5])
def test_a_bad_scale_is_refused_before_anything_is_created(tmp_path, bad):
    p = _level0(tmp_path)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="only scale factors"):
        zd.destripe_zarr_store(p, str(out / "g" / "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                               prediction_chunksize=(4, 16, 16), output_chunks=(1, 1, 2, 8, 8), compressor=None,
                               pyramid_group=str(out / "g"), n_levels=3, scale_factor=bad)  # fmt: skip
    with pytest.raises(ValueError, match="only scale factors"):
        zd.destripe_zarr(dataset_path=p, multiscale="0", output_destriped_zarr=out / "tile.zarr", prediction_chunksize=(4, 16, 16),
                         target_size_mb=3072, n_workers=0, batch_size=1, super_chunksize=(8, 16, 16),
                         results_folder=out / "results", derivatives_path=out / "nowhere", xyz_resolution=[1.8, 1.8, 2.0],
                         parameters={"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG},
                         output_chunks=(1, 1, 2, 8, 8), fused_pyramid=True, scale_factor=bad)  # fmt: skip
    with pytest.raises(ValueError, match="only scale factors"):
        zd.destripe_channel(zarr_dataset_path=tmp_path, derivatives_path=out / "nowhere", channel_name="c", results_folder=out / "results",
                            xyz_resolution=[1.8, 1.8, 2.0], estimated_channel_flats=[], laser_tiles={}, parameters={},
                            scale_factor=bad)  # fmt: skip
    for kw in ({}, {"pipelined": True}):
        with pytest.raises(ValueError, match="only scale factors"):
            zd.compute_multiscale(p, str(out / "g"), bad, 1, [2.0, 1.8, 1.8], "t", n_levels=3, chunks=(1, 1, 2, 8, 8),
                                  compressor=None, ome_metadata=True, **kw)  # fmt: skip
    with pytest.raises(ValueError, match="only scale factors"):
        pyramid.write_pyramid_levels(p, str(out / "g"), scale_factor=bad, compressor=None)
    assert not out.exists()


def test_the_new_keyword_is_keyword_only_and_optional():
    for fn, default in ((zd.destripe_zarr_store, (2, 2, 2)), (zd.destripe_zarr, None), (zd.destripe_channel, None)):
        p = inspect.signature(fn).parameters["scale_factor"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default, fn


def test_ome_scales_follow_the_factor_per_axis():
    transforms, chunk_sizes = zd._compute_scales(4, [1, 2, 2], (2.0, 1.8, 1.8), (1, 1, 64, 128, 128), (1, 1, 100, 400, 600))
    assert len(transforms) == 4
    for lvl, entry in enumerate(transforms):
        assert entry == [{"type": "scale", "scale": [1.0, 1.0, 2.0, 1.8 * 2**lvl, 1.8 * 2**lvl]}], lvl
    assert [c["chunks"] for c in chunk_sizes] == [(1, 1, 64, 128, 128), (1, 1, 64, 128, 128), (1, 1, 64, 100, 128), (1, 1, 64, 50, 75)]


def test_host_builds_under_sanitizers(tmp_path):
    """tests/host/pyramid_scale_check.cpp with ASan / UBSan: the block, the source bricks and every level live in heap
    buffers of exactly their own size; odd extents, tail chunks, a z offset, both host builds, every factor set."""
    exe = str(tmp_path / "pyramid_scale_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "pyramid_scale_check.cpp")], check=True)  # fmt: skip
    for zyx, base, z0, src_chunk in (((7, 9, 11), (3, 5, 7), 2, (3, 5, 7)), ((8, 20, 44), (4, 8, 8), 0, (4, 8, 8)),
                                     ((6, 10, 12), (5, 3, 5), 4, (4, 16, 5))):  # fmt: skip
        vol = pc.block_volume(zyx)
        raw = str(tmp_path / "block.raw")
        vol.tofile(raw)
        for scale in pc.SCALES:
            want, n_levels = [], 4
            for lvl, lv in enumerate(fo.pyramid(vol, n_levels, scale)[1:], start=1):
                if min(lv.shape) == 0:
                    break
                ck = (base[0], min(base[1], lv.shape[1]), min(base[2], lv.shape[2]))
                want.append(fo.planes_to_bricks(lv, ck, z0))
            assert want
            for sc in ((0, 0, 0), src_chunk):
                res = str(tmp_path / "res.out")
                run = subprocess.run([exe, raw, *map(str, zyx), *map(str, scale), str(n_levels), *map(str, base), str(z0),
                                      *map(str, sc), res], capture_output=True, text=True)  # fmt: skip
                assert run.returncode == 0, (zyx, scale, sc, run.stderr[-2000:])
                got = np.fromfile(res, np.uint16)
                assert got.tobytes() == b"".join(w.tobytes() for w in want), (zyx, scale, sc)
