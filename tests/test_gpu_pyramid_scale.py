"""The pyramid with a scale factor of 1 or 2 per axis on the device: ``k_pyramid_step`` (``dsx_pyramid_block_scale_u16``
/ ``dsx_pyramid_bricks_scale_u16``) against the host builds, byte for byte, ``compute_pyramid`` against the oracle, and
the stores of the three routes -- slabs, ``pipelined=True``, the fused pass -- against each other and the oracle."""

import json
import os
import shutil

import numpy as np
import pytest

import pyramid_scale_cases as pc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import pyramid, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import format_oracle as fo

pytestmark = pytest.mark.gpu
SCALES = pytest.mark.parametrize("scale", pc.SCALES, ids=pc.scale_id)

# (block, base chunk of the levels, source chunk): the vector body; two tail shapes (odd extents, odd chunks); columns
# that would vectorise under a chunk cx that holds no whole store
KERNEL_CASES = [((8, 32, 64), (4, 16, 16), (4, 16, 16)), ((7, 9, 11), (3, 5, 7), (3, 5, 7)), ((6, 10, 12), (3, 5, 7), (3, 5, 7)),
                ((8, 12, 32), (4, 6, 7), (4, 6, 8))]  # fmt: skip


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _pattern(shape):
    return ((np.arange(int(np.prod(shape)), dtype=np.uint32) * 7 + 0x8001) & 0xFFFF).astype(np.uint16).reshape(shape)


@SCALES
def test_step_kernels_equal_the_host_build(eng, scale):
    """Dense and brick source, three levels, z offsets inside rows that hold more than the share; the outputs are
    pre-filled with a pattern and not zeroed (``zero=False``), so every position outside the share must keep it."""
    for zyx, base, src_chunk in KERNEL_CASES:
        vol = pc.block_volume(zyx)
        chunks = pc.level_chunks(zyx, base, 4, scale, vol_z=4096)
        n = len(chunks)
        assert n >= 2
        src = pc.source_bricks(vol, src_chunk)
        work = eng_mod.pyramid_work_bytes(zyx, n + 1, scale)
        bufs = [eng.alloc(vol.nbytes), eng.alloc(src.nbytes)] + ([eng.alloc(work)] if work else [])
        d_vol, d_src, d_work = bufs[0], bufs[1], bufs[2] if work else None
        try:
            d_vol.upload(vol)
            d_src.upload(src)
            for z0s in ([0] * n, [3, 2, 1][:n]):
                share = [pc.extents(zyx, l, scale)[0] for l in range(1, n + 1)]
                rows = [-(-(z0 + s) // c[0]) + (1 if z0 else 0) for z0, s, c in zip(z0s, share, chunks)]
                shapes = [g.shape for g in eng_mod.pyramid_block_ref(vol, chunks, z0s=z0s, rows=rows, scale=scale)]
                for dense in (True, False):
                    ref = [_pattern(s) for s in shapes]
                    if dense:
                        eng_mod.pyramid_block_ref(vol, chunks, z0s=z0s, bricks=ref, rows=rows, scale=scale)
                    else:
                        eng_mod.pyramid_bricks_ref(src, zyx, src_chunk, chunks, z0s=z0s, bricks_out=ref, rows=rows, scale=scale)
                    assert all((r != _pattern(r.shape)).any() for r in ref)
                    if z0s[0]:  # (the spare row: nothing of it belongs to the share)
                        assert all((r[-1] == _pattern(r.shape)[-1]).all() for r in ref)
                    d_bricks = [eng.alloc(max(r.nbytes, 16)) for r in ref]
                    try:
                        for b, r in zip(d_bricks, ref):
                            b.upload(_pattern(r.shape))
                        kw = dict(z0s=z0s, zero=[False] * n, rows=rows, d_work=d_work, scale=scale)
                        if dense:
                            eng.pyramid_block(d_vol, zyx, chunks, d_bricks, **kw)
                        else:
                            eng.pyramid_bricks(d_src, zyx, src_chunk, chunks, d_bricks, **kw)
                        eng.sync()
                        for lvl, (b, r) in enumerate(zip(d_bricks, ref), start=1):
                            got = b.download((r.size,), np.uint16)
                            assert got.tobytes() == r.tobytes(), (zyx, scale, chunks, z0s, dense, lvl)
                    finally:
                        for b in d_bricks:
                            b.free()
        finally:
            for b in bufs:
                b.free()


def test_compute_pyramid_equals_the_oracle(eng):
    vol = pc.block_volume((12, 40, 64))
    got = zd.compute_pyramid(vol[None, None], 4, (1, 1, 1, 2, 2), engine=eng)
    want = fo.pyramid(vol, 4, (1, 2, 2))
    assert [g.shape for g in got] == [(1, 1) + w.shape for w in want] == [(1, 1, 12, 40 >> l, 64 >> l) for l in range(4)]
    assert all(np.array_equal(g[0, 0], w) for g, w in zip(got, want))
    for zyx in ((12, 40, 64), (9, 21, 43)):  # the vector body and the tail body of the dense step
        vol = pc.block_volume(zyx)
        for scale in pc.SCALES:
            want = [w for w in fo.pyramid(vol, 4, scale) if min(w.shape)]
            if scale[1] == scale[2]:  # (compute_pyramid reduces y and x alike)
                got = pyramid.compute_pyramid(vol, 4, scale, engine=eng)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (zyx, scale)
            # the dense one-level reduce that the slab route runs, every scale: level 1 from level 0, level 2 from 1
            for src, dst in zip(want[:2], want[1:3]):
                d_src, d_dst = eng.alloc(src.nbytes), eng.alloc(max(dst.nbytes, 16))
                try:
                    d_src.upload(src)
                    eng.downsample2(d_src, d_dst, src.shape, scale)
                    eng.sync()
                    assert np.array_equal(d_dst.download(dst.shape, np.uint16), dst), (zyx, scale, src.shape)
                finally:
                    d_src.free()
                    d_dst.free()


def _chunk_files(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs if not f.startswith("."))


def _assert_same_levels(a, b, n_levels, first=1):
    for lvl in range(first, n_levels):
        pa, pb = os.path.join(a, str(lvl)), os.path.join(b, str(lvl))
        with open(os.path.join(pa, ".zarray")) as fa, open(os.path.join(pb, ".zarray")) as fb:
            assert json.load(fa) == json.load(fb), (b, lvl)
        assert _chunk_files(pa) == _chunk_files(pb), (b, lvl)
        assert np.array_equal(MiniZarrArray.open(pa)[0, 0], MiniZarrArray.open(pb)[0, 0]), (b, lvl)
    assert not os.path.exists(os.path.join(b, str(n_levels))) and not os.path.exists(os.path.join(a, str(n_levels)))


Z, H, W, CHUNKS = 16, 32, 48, (1, 1, 4, 16, 16)


@pytest.fixture(scope="module")
def level0(tmp_path_factory):
    """The input store, and level 0 of a run without a pyramid (Blosc, host codec): what every route starts from."""
    root = tmp_path_factory.mktemp("pyramid_scale")
    in_path = str(root / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(in_path, (1, 1, Z, H, W), CHUNKS, np.uint16, compressor="blosc")
    src[0, 0] = synth.synthetic_stack(Z, H, W, n_unique=4)
    plain = str(root / "plain")
    try:
        n, _ = zd.destripe_zarr_store(in_path, os.path.join(plain, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                      prediction_chunksize=(4, H, W), output_chunks=CHUNKS, device=0, device_retile=True,
                                      io_threads=4)  # fmt: skip
        assert n == Z and zd.LAST_RUN["pyramid_scale"] is None
    finally:
        zd.release_staging()
    return root, in_path, plain


@pytest.mark.parametrize("scale", [(1, 2, 2), (2, 1, 1), (2, 2, 1)], ids=pc.scale_id)
def test_the_three_routes_write_the_same_stores(level0, scale):
    root, in_path, plain = level0
    tag, n_levels = pc.scale_id(scale), 3
    groups = {k: str(root / (k + "_" + tag)) for k in ("slabs", "pipelined", "pipelined_device", "fused")}
    for k in ("slabs", "pipelined", "pipelined_device"):
        shutil.copytree(os.path.join(plain, "0"), os.path.join(groups[k], "0"))
    kw = dict(n_levels=n_levels, chunks=CHUNKS, compressor="blosc", device=0)
    shapes = zd.compute_multiscale(os.path.join(groups["slabs"], "0"), groups["slabs"], list(scale), 1, None, "t", **kw)
    want_shapes = [(1, 1) + pc.extents((Z, H, W), l, scale) for l in (1, 2)]
    assert shapes == want_shapes and pyramid.LAST_PYRAMID["route"] == "slabs" and pyramid.LAST_PYRAMID["scale"] == scale
    for k, extra in (("pipelined", {}), ("pipelined_device", dict(device_codec="runs", device_decode=True))):
        g = groups[k]
        assert zd.compute_multiscale(os.path.join(g, "0"), g, list(scale), 1, None, "t", pipelined=True, io_threads=4,
                                     **extra, **kw) == want_shapes  # fmt: skip
        last = pyramid.LAST_PYRAMID
        assert last["route"] == "pipelined" and last["block_z"] == 4 and last["scale"] == scale and last["levels"] == [1, 2]
        assert last["decode_routes"]["device" if extra else "host"] == 4 * 2 * 3
    try:
        g = groups["fused"]
        n, _ = zd.destripe_zarr_store(in_path, os.path.join(g, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                      prediction_chunksize=(4, H, W), output_chunks=CHUNKS, device=0, device_retile=True,
                                      io_threads=4, pyramid_group=g, n_levels=n_levels, scale_factor=scale)  # fmt: skip
        assert n == Z and zd.LAST_RUN["fused_pyramid"] is True and zd.LAST_RUN["pyramid_levels"] == [1, 2]
        assert zd.LAST_RUN["pyramid_scale"] == scale
    finally:
        zd.release_staging()
    # level 0 of the fused run is, byte for byte, that of the run without a pyramid
    files = _chunk_files(os.path.join(plain, "0"))
    assert files == _chunk_files(os.path.join(groups["fused"], "0")) and len(files) == 4 * 2 * 3
    for f in files + [".zarray"]:
        with open(os.path.join(plain, "0", f), "rb") as fa, open(os.path.join(groups["fused"], "0", f), "rb") as fb:
            assert fa.read() == fb.read(), f
    for k in ("pipelined", "pipelined_device", "fused"):
        _assert_same_levels(groups["slabs"], groups[k], n_levels)
    want = fo.pyramid(MiniZarrArray.open(os.path.join(plain, "0"))[0, 0], n_levels, scale)
    for k, g in groups.items():
        for lvl in (1, 2):
            arr = MiniZarrArray.open(os.path.join(g, str(lvl)))
            assert arr.chunks == (1, 1) + tuple(min(c, n) for c, n in zip(CHUNKS[-3:], want[lvl].shape)), (k, lvl)
            assert np.array_equal(arr[0, 0], want[lvl]), (k, lvl)


def test_destripe_zarr_fused_with_a_scale_writes_the_group_of_the_default_call(tmp_path):
    """``destripe_zarr(scale_factor=[1, 2, 2], ome_metadata=True)`` with and without ``fused_pyramid``: the same arrays,
    chunk files, voxels and ``.zattrs``, whose scales follow the factor per axis."""
    tile = tmp_path / "data" / "X_0_Y_0.zarr"
    a = MiniZarrArray.create(str(tile / "0"), (1, 1, Z, H, W), CHUNKS, np.uint16, compressor="blosc")
    a[0, 0] = synth.synthetic_stack(Z, H, W, n_unique=4)
    common = dict(dataset_path=tile, multiscale="0", prediction_chunksize=(4, H, W), target_size_mb=3072, n_workers=0,
                  batch_size=1, super_chunksize=(8, H, W), results_folder=tmp_path / "results",
                  derivatives_path=tmp_path / "nowhere", xyz_resolution=[1.8, 1.8, 2.0],
                  parameters={"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}, flatfield=None,
                  lazy_callback_fn=None, device=0, output_chunks=CHUNKS, n_levels=3, io_threads=4, ome_metadata=True,
                  scale_factor=[1, 2, 2])  # fmt: skip
    ga, gb = (tmp_path / n / "X_0_Y_0.zarr" for n in ("default", "fused"))
    try:
        n, _ = zd.destripe_zarr(output_destriped_zarr=ga, **common)
        assert n == Z and pyramid.LAST_PYRAMID["scale"] == (1, 2, 2) and zd.LAST_RUN["pyramid_scale"] == (1, 2, 2)
        n, _ = zd.destripe_zarr(output_destriped_zarr=gb, fused_pyramid=True, **common)
        assert n == Z and zd.LAST_RUN["fused_pyramid"] is True and zd.LAST_RUN["pyramid_scale"] == (1, 2, 2)
    finally:
        zd.release_staging()
    _assert_same_levels(str(ga), str(gb), 3, first=0)
    with open(ga / ".zattrs") as fa, open(gb / ".zattrs") as fb:
        attrs = json.load(fa)
        assert attrs == json.load(fb)
    with open(ga / ".zgroup") as fa, open(gb / ".zgroup") as fb:
        assert json.load(fa) == json.load(fb)
    datasets = attrs["multiscales"][0]["datasets"]
    assert [d["coordinateTransformations"][0]["scale"] for d in datasets] == [[1.0, 1.0, 2.0, 1.8 * 2**l, 1.8 * 2**l]
                                                                              for l in range(3)]  # fmt: skip
    want = fo.pyramid(MiniZarrArray.open(str(gb / "0"))[0, 0], 3, (1, 2, 2))
    for lvl in (1, 2):
        assert np.array_equal(MiniZarrArray.open(str(gb / str(lvl)))[0, 0], want[lvl]), lvl
