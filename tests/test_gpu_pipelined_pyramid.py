"""The stand-alone pyramid in one pipelined device pass (``compute_multiscale(pipelined=True)``):
``dsx_pyramid_bricks_u16`` on the device against its host build, byte for byte, and the stores of the pipelined route
against the default route's: same ``.zarray``, same chunk files, same voxels at every level, read back by the host."""

import json
import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import pyramid, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import format_oracle as fo
from test_gpu_fused_pyramid import _corrupt
from test_pyramid_bricks_host import BLOCKS, SRC_CHUNKS, block_volume, level_chunk_cases, source_bricks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("zyx", BLOCKS)
def test_pyramid_bricks_on_the_device_is_the_host_build(zyx):
    """Every block / source chunk / level case of the host test, the source padding poisoned, the output buffers
    pre-filled with 0xFFFF (the zeroing of a fresh row is the call's own), at two z offsets inside the chunk rows.
    Source chunks (3, 5, 7) and the odd extents take the tail path, the others the vector path."""
    vol = block_volume(zyx)
    e = eng_mod.DestripeEngine(0)
    bufs = []
    try:
        for sc in SRC_CHUNKS:
            src = source_bricks(vol, sc, poison=True)
            d_src = e.alloc(src.nbytes)
            bufs.append(d_src)
            d_src.upload(src)
            for chunks in level_chunk_cases(zyx):
                n = len(chunks)
                work = eng_mod.pyramid_work_bytes(zyx, n + 1)
                d_work = e.alloc(work) if work else None
                for off1 in (0, 32):  # z offset inside the level-1 row (and half of it inside the level-2 row, ...)
                    z0s = [off1 >> l for l in range(n)]
                    rows = [-(-(z0 + (zyx[0] >> l)) // c[0]) for l, (z0, c) in enumerate(zip(z0s, chunks), start=1)]
                    ref = eng_mod.pyramid_bricks_ref(src, zyx, sc, chunks, z0s=z0s, rows=rows)
                    d_bricks = [e.alloc(max(r.nbytes, 16)) for r in ref]
                    try:
                        for b, r in zip(d_bricks, ref):
                            b.upload(np.full(max(r.size, 8), 0xFFFF, np.uint16))
                        e.pyramid_bricks(d_src, zyx, sc, chunks, d_bricks, z0s=z0s, rows=rows, d_work=d_work)
                        e.sync()
                        for lvl, (b, r) in enumerate(zip(d_bricks, ref), start=1):
                            got = b.download((r.size,), np.uint16)
                            assert got.tobytes() == r.tobytes(), (zyx, sc, chunks, off1, lvl)
                    finally:
                        for b in d_bricks:
                            b.free()
                if d_work is not None:
                    d_work.free()
    finally:
        for b in bufs:
            b.free()
        e.close()


def _chunk_files(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs if not f.startswith("."))


def _assert_same_stores(a, b, n_levels, first=1):
    """Groups ``a`` (default route) and ``b`` (pipelined): metadata, chunk file names and voxels of every level, the
    voxels against the oracle's pyramid of level 0, and no level ``n_levels``."""
    for lvl in range(first, n_levels):
        pa, pb = os.path.join(a, str(lvl)), os.path.join(b, str(lvl))
        with open(os.path.join(pa, ".zarray")) as fa, open(os.path.join(pb, ".zarray")) as fb:
            assert json.load(fa) == json.load(fb), lvl
        assert _chunk_files(pa) == _chunk_files(pb), lvl
        assert np.array_equal(MiniZarrArray.open(pa)[0, 0], MiniZarrArray.open(pb)[0, 0]), lvl
    assert not os.path.exists(os.path.join(b, str(n_levels))) and not os.path.exists(os.path.join(a, str(n_levels)))
    pyr = fo.pyramid(MiniZarrArray.open(os.path.join(b, "0"))[0, 0], n_levels)
    for lvl in range(1, n_levels):
        assert np.array_equal(MiniZarrArray.open(os.path.join(b, str(lvl)))[0, 0], pyr[lvl]), lvl


def _volume(Z, H, W):
    rs = np.random.RandomState(Z + H + W)
    vol = synth.synthetic_stack(Z, H, W, n_unique=4).astype(np.uint16)
    vol[:, : H // 3, : W // 3] = 0x1200 + rs.randint(0, 256, (Z, H // 3, W // 3))  # a corner with noise in the low bytes
    return vol


def _write_level0(group, vol, chunks, compressor):
    a = MiniZarrArray.create(os.path.join(group, "0"), (1, 1) + vol.shape, chunks, np.uint16, compressor=compressor)
    a[0, 0] = vol
    return a


def _multiscale(group, n_levels, chunks, compressor, **kw):
    return zd.compute_multiscale(os.path.join(group, "0"), group, [2, 2, 2], 1, None, "t", n_levels=n_levels, chunks=chunks,
                                 compressor=compressor, device=0, **kw)  # fmt: skip


GEOMETRY_1 = ((160, 200, 312), (1, 1, 64, 128, 128))


@pytest.fixture(scope="module")
def first_geometry(tmp_path_factory):
    """Level 0 of the first geometry (Blosc), written once, and the default route's pyramid per ``n_levels``."""
    root = tmp_path_factory.mktemp("pipelined_g1")
    vol = _volume(*GEOMETRY_1[0])
    groups = {}
    for n_levels in (3, 4):
        a = str(root / "default_{}".format(n_levels))
        _write_level0(a, vol, GEOMETRY_1[1], "blosc")
        _multiscale(a, n_levels, GEOMETRY_1[1], "blosc")
        assert pyramid.LAST_PYRAMID["route"] == "slabs"
        groups[n_levels] = a
    return root, vol, groups


@pytest.mark.parametrize("n_levels", [3, 4])
@pytest.mark.parametrize("decode,codec", [(False, False), (True, True), ("any", "runs")])
def test_pipelined_store_equals_the_default_route(first_geometry, n_levels, decode, codec):
    """Edge chunks in y and x, a level-1 row that leaves after two blocks, a 32-plane last block, half a row that leaves
    at the end, clamped chunks at levels 2 and 3."""
    root, vol, groups = first_geometry
    b = str(root / "pipelined_{}_{}_{}".format(n_levels, decode, codec))
    _write_level0(b, vol, GEOMETRY_1[1], "blosc")
    shapes = _multiscale(b, n_levels, GEOMETRY_1[1], "blosc", pipelined=True, device_decode=decode, device_codec=codec,
                         io_threads=8)  # fmt: skip
    assert shapes == [(1, 1, 80, 100, 156), (1, 1, 40, 50, 78), (1, 1, 20, 25, 39)][: n_levels - 1]
    last = dict(pyramid.LAST_PYRAMID)
    assert last["route"] == "pipelined" and last["block_z"] == 64 and last["levels"] == list(range(1, n_levels))
    n_chunks = 3 * 2 * 3
    assert sum(last["decode_routes"].values()) == n_chunks
    assert last["decode_routes"] == ({"device": n_chunks, "host": 0, "fill": 0} if decode else
                                     {"device": 0, "host": n_chunks, "fill": 0})  # fmt: skip
    assert last["upload_bytes"] > 0 and last["download_bytes"] > 0 and last["seconds"] > 0
    _assert_same_stores(groups[n_levels], b, n_levels)
    assert MiniZarrArray.open(os.path.join(b, "2")).chunks == (1, 1, 40, 50, 78)


@pytest.mark.parametrize("compressor", [None, "zlib"])
def test_pipelined_store_odd_extents_raw_and_zlib(tmp_path, compressor):
    """Odd extents on every axis, source chunks (16, 32, 32): the tail path of the kernel, ten blocks, host writers."""
    vol, chunks = _volume(150, 203, 301), (1, 1, 16, 32, 32)
    a, b = str(tmp_path / "default"), str(tmp_path / "pipelined")
    for g in (a, b):
        _write_level0(g, vol, chunks, compressor)
    _multiscale(a, 4, chunks, compressor)
    _multiscale(b, 4, chunks, compressor, pipelined=True, io_threads=8)
    assert pyramid.LAST_PYRAMID["route"] == "pipelined" and pyramid.LAST_PYRAMID["block_z"] == 16
    _assert_same_stores(a, b, 4)


@pytest.mark.parametrize("how", ["truncated", "reserved bit"])
def test_bad_chunk_raises_naming_it_and_no_row_with_its_data_is_written(tmp_path, how):
    """Four blocks of one chunk row each; the bad chunk file belongs to block 2: level-1 row 1 (blocks 2 and 3) and the
    one row of level 2 hold its data and must not appear.  A file cut short is refused by the reader, a broken zstd
    frame header by the device decoder (its status)."""
    vol, chunks = _volume(256, 128, 256), (1, 1, 64, 128, 128)
    g = str(tmp_path / "g")
    src = _write_level0(g, vol, chunks, "blosc")
    victim = src._chunk_path((0, 0, 2, 0, 1))
    with open(victim, "rb") as fh:
        frame = fh.read()
    if how == "truncated":
        with open(victim, "wb") as fh:
            fh.write(frame[: 16 + (len(frame) - 16) // 2])  # in the middle of its compressed stream
    else:
        _corrupt(victim)
    with pytest.raises(ValueError) as ei:
        _multiscale(g, 3, chunks, "blosc", pipelined=True, device_decode=True, io_threads=8)
    assert victim in str(ei.value), str(ei.value)
    row0 = {os.path.join("0", "0", "0", str(y), str(x)) for y in range(1) for x in range(1)}
    assert set(_chunk_files(os.path.join(g, "1"))) <= row0
    assert _chunk_files(os.path.join(g, "2")) == []
    with open(victim, "wb") as fh:  # and a good run follows
        fh.write(frame)
    _multiscale(g, 3, chunks, "blosc", pipelined=True, device_decode=True, io_threads=8)
    pyr = fo.pyramid(vol, 3)
    for lvl in (1, 2):
        assert np.array_equal(MiniZarrArray.open(os.path.join(g, str(lvl)))[0, 0], pyr[lvl]), lvl


def test_destripe_zarr_with_the_pipelined_pyramid_equals_the_default_call(tmp_path):
    """The whole route on a 96 x 128 tile of 128 planes: ``destripe_zarr(..., pipelined_pyramid=True)`` against the
    reference's call; level 0 is byte-identical on disk (the host codec wrote both)."""
    H, W, Z = 96, 128, 128
    tile = tmp_path / "data" / "X_0_Y_0.zarr"
    a = MiniZarrArray.create(str(tile / "0"), (1, 1, Z, H, W), (1, 1, 64, 32, 32), np.uint16, compressor="blosc")
    a[0, 0] = synth.synthetic_stack(Z, H, W, n_unique=4)
    common = dict(dataset_path=tile, multiscale="0", prediction_chunksize=(64, H, W), target_size_mb=3072, n_workers=0,
                  batch_size=1, super_chunksize=(384, H, W), results_folder=tmp_path / "results",
                  derivatives_path=tmp_path / "nowhere", xyz_resolution=[1.8, 1.8, 2.0],
                  parameters={"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}, flatfield=None,
                  lazy_callback_fn=None, device=0, output_chunks=(1, 1, 64, 32, 32), n_levels=3, io_threads=8)  # fmt: skip
    ga, gb, gc = (tmp_path / n / "X_0_Y_0.zarr" for n in ("default", "pipelined", "pipelined_codecs"))
    try:
        n, _ = zd.destripe_zarr(output_destriped_zarr=ga, **common)
        assert n == Z and pyramid.LAST_PYRAMID["route"] == "slabs"
        n, _ = zd.destripe_zarr(output_destriped_zarr=gb, pipelined_pyramid=True, **common)
        assert n == Z and pyramid.LAST_PYRAMID["route"] == "pipelined"
        assert pyramid.LAST_PYRAMID["decode_routes"]["device"] == 0
        _assert_same_stores(str(ga), str(gb), 3, first=0)
        for f in _chunk_files(str(ga / "0")):
            with open(ga / "0" / f, "rb") as fa, open(gb / "0" / f, "rb") as fb:
                assert fa.read() == fb.read(), f
        n, _ = zd.destripe_zarr(output_destriped_zarr=gc, pipelined_pyramid=True, device_codec="runs", device_decode=True,
                                **common)  # fmt: skip
        routes = pyramid.LAST_PYRAMID["decode_routes"]  # (level 0 holds the device encoder's frames here)
        assert n == Z and sum(routes.values()) == 2 * 3 * 4 and routes["fill"] == 0 and routes["device"] > 0
        _assert_same_stores(str(ga), str(gc), 3, first=0)
    finally:
        zd.release_staging()
