"""The pyramid levels built in the destripe pass (``fused_pyramid``): ``dsx_pyramid_block_u16`` on the device against
its host build, byte for byte, and ``destripe_zarr_store(pyramid_group=..., n_levels=...)`` against the two-pass route
(``destripe_zarr_store`` then ``compute_multiscale``): same ``.zarray``, same chunk files, same voxels at every level."""

import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_tiff, pyramid, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import format_oracle as fo

pytestmark = pytest.mark.gpu


def _device_levels(e, vol, chunks, z0s, rows):
    """``pyramid_block`` into buffers pre-filled with 0xFFFF (so the zeroing of a fresh row is the call's own)."""
    n = len(chunks)
    sizes = [eng_mod.pyramid_level_elems(vol.shape, l + 1, chunks[l], rows[l]) for l in range(n)]
    d_vol = e.alloc(vol.nbytes)
    d_bricks = [e.alloc(max(s * 2, 16)) for s in sizes]
    work = eng_mod.pyramid_work_bytes(vol.shape, n + 1)
    d_work = e.alloc(work) if work else None
    try:
        d_vol.upload(vol)
        for b, s in zip(d_bricks, sizes):
            b.upload(np.full(max(s, 8), 0xFFFF, np.uint16))
        e.pyramid_block(d_vol, vol.shape, chunks, d_bricks, z0s=z0s, rows=rows, d_work=d_work)
        e.sync()
        return [b.download((s,), np.uint16) for b, s in zip(d_bricks, sizes)]
    finally:
        for b in [d_vol, d_work] + d_bricks:
            if b is not None:
                b.free()


def test_pyramid_block_on_the_device_is_the_host_build():
    rs = np.random.RandomState(3)
    cases = []
    for zyx in ((64, 36, 50), (8, 20, 44), (6, 10, 12), (64, 256, 384)):
        for L in (2, 3, 4, 5):
            for base in ((64, 128, 128), (4, 8, 8), (3, 5, 7)):
                for vol_z in (zyx[0], 4096):  # clamped / unclamped z chunks
                    chunks = [lv.chunks for lv in pyramid.fused_levels((vol_z,) + zyx[1:], base, L)]
                    chunks = [c for l, c in enumerate(chunks, start=1) if zyx[0] >> l and zyx[1] >> l and zyx[2] >> l]
                    if chunks:
                        cases.append((zyx, chunks))
    cases += [((64, 2048, 2048), [(64, 128, 128), (64, 128, 128)]), ((64, 1600, 2000), [(64, 128, 128), (64, 128, 128)]),
              ((64, 1600, 2000), [(48, 128, 128), (24, 128, 128), (12, 100, 125)])]  # fmt: skip
    e = eng_mod.DestripeEngine(0)
    try:
        for zyx, chunks in cases:
            vol = rs.randint(0, 65536, zyx).astype(np.uint16)
            vol[: zyx[0] // 2, : zyx[1] // 2] |= 0xFFF0
            for off1 in (0, 32):  # z offset inside the level-1 row (and half of it inside the level-2 row)
                z0s = [off1 >> l for l in range(len(chunks))]
                rows = [-(-(z0 + (zyx[0] >> l)) // c[0]) for l, (z0, c) in enumerate(zip(z0s, chunks), start=1)]
                ref = eng_mod.pyramid_block_ref(vol, chunks, z0s=z0s, rows=rows)
                got = _device_levels(e, vol, chunks, z0s, rows)
                for lvl, (g, r) in enumerate(zip(got, ref), start=1):
                    assert g.tobytes() == r.tobytes(), (zyx, chunks, off1, lvl)
    finally:
        e.close()


def _chunk_files(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs if not f.startswith("."))


def _assert_same_stores(a, b, n_levels):
    """Groups ``a`` (two-pass) and ``b`` (fused): metadata, chunk file names and voxels of every level."""
    for lvl in range(n_levels):
        pa, pb = os.path.join(a, str(lvl)), os.path.join(b, str(lvl))
        with open(os.path.join(pa, ".zarray")) as fa, open(os.path.join(pb, ".zarray")) as fb:
            assert json.load(fa) == json.load(fb), lvl
        assert _chunk_files(pa) == _chunk_files(pb), lvl
        assert np.array_equal(MiniZarrArray.open(pa)[0, 0], MiniZarrArray.open(pb)[0, 0]), lvl
    assert not os.path.exists(os.path.join(b, str(n_levels))) and not os.path.exists(os.path.join(a, str(n_levels)))
    pyr = fo.pyramid(MiniZarrArray.open(os.path.join(b, "0"))[0, 0], n_levels)
    for lvl in range(1, n_levels):
        assert np.array_equal(MiniZarrArray.open(os.path.join(b, str(lvl)))[0, 0], pyr[lvl]), lvl


def _make_input(tmp_path, Z, H, W, chunks=(1, 1, 64, 128, 128), compressor="blosc"):
    vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, Z, H, W), chunks, np.uint16, compressor=compressor)
    for z in range(0, Z, 64):
        src[0, 0, z : z + 64] = vol[z : z + 64]
    return path, src


def _both_routes(tmp_path, in_path, tag, n_levels, block, chunks, compressor, sc=None, **kw):
    """Run A: level 0, then ``compute_multiscale``; run B: one call with the fused option.  Returns the two groups."""
    a, b = str(tmp_path / ("two_pass_" + tag)), str(tmp_path / ("fused_" + tag))
    common = dict(prediction_chunksize=block, output_chunks=chunks, device=0, device_retile=True, compressor=compressor,
                  io_threads=16, **kw)  # fmt: skip
    Z = MiniZarrArray.open(in_path).shape[-3]
    n, _ = zd.destripe_zarr_store(in_path, os.path.join(a, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, sc, **common)
    assert n == Z and zd.LAST_RUN["fused_pyramid"] is False
    zd.compute_multiscale(os.path.join(a, "0"), a, [2, 2, 2], 1, None, "t", n_levels=n_levels, chunks=chunks,
                          compressor=compressor, device=0)  # fmt: skip
    n, _ = zd.destripe_zarr_store(in_path, os.path.join(b, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, sc,
                                  pyramid_group=b, n_levels=n_levels, **common)  # fmt: skip
    assert n == Z and zd.LAST_RUN["fused_pyramid"] is True
    return a, b


def test_fused_store_equals_two_pass_2048(tmp_path):
    """192 planes of 2048^2 = three z blocks: the first level-1 chunk row completes after two, half a row leaves at the
    end; level 2 (48 planes, one clamped chunk row) leaves once.  All four codec placements."""
    in_path, _ = _make_input(tmp_path, 192, 2048, 2048)
    try:
        for codec in (False, True):
            for decode in (False, True):
                a, b = _both_routes(tmp_path, in_path, "{}{}".format(int(codec), int(decode)), 3, (64, 2048, 2048),
                                    (1, 1, 64, 128, 128), "blosc", device_codec=codec, device_decode=decode)  # fmt: skip
                assert zd.LAST_RUN["pyramid_levels"] == [1, 2]
                assert zd._BLOCKS["blocks"][1].timing["pyramid_download_bytes"] > 0
                _assert_same_stores(a, b, 3)
                assert MiniZarrArray.open(os.path.join(b, "2")).chunks == (1, 1, 48, 128, 128)
    finally:
        zd.release_staging()


def test_fused_store_equals_two_pass_production_tile(tmp_path):
    """1600 x 2000, 96 planes (a ragged last z block), shading on, four levels (level 3 comes from the plain per-level
    kernel and has a clamped chunk shape), both codecs on the device."""
    H, W = 1600, 2000
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.15 * (((yy - H / 2.0) / (H / 2.0)) ** 2 + ((xx - W / 2.0) / (W / 2.0)) ** 2)).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": np.full((H, W), 100.0, np.float32)}
    in_path, _ = _make_input(tmp_path, 96, H, W)
    try:
        a, b = _both_routes(tmp_path, in_path, "prod", 4, (64, H, W), (1, 1, 64, 128, 128), "blosc", sc=sc,
                            device_codec=True, device_decode=True)  # fmt: skip
        assert zd.LAST_RUN["pyramid_levels"] == [1, 2, 3]
        _assert_same_stores(a, b, 4)
        assert MiniZarrArray.open(os.path.join(b, "3")).chunks == (1, 1, 12, 128, 128)
    finally:
        zd.release_staging()


@pytest.mark.parametrize("compressor", [None, "zlib"])
def test_fused_store_with_host_writers_raw_and_zlib(tmp_path, compressor):
    try:
        in_path, _ = _make_input(tmp_path, 128, 256, 384, compressor=compressor)
        a, b = _both_routes(tmp_path, in_path, "big", 3, (64, 256, 384), (1, 1, 64, 128, 128), compressor)
        _assert_same_stores(a, b, 3)
        small = tmp_path / "small"
        small.mkdir()
        in_path, _ = _make_input(small, 24, 64, 96, chunks=(1, 1, 4, 32, 32), compressor=compressor)
        a, b = _both_routes(small, in_path, "small", 3, (4, 64, 96), (1, 1, 4, 32, 32), compressor)
        _assert_same_stores(a, b, 3)
    finally:
        zd.release_staging()


def test_two_ranks_fused_equal_one_rank_two_pass(tmp_path):
    """Two processes, one per rank, both on this box's one GPU, through ``destripe_channel`` with a ``RankGroup``: every
    rank writes the pyramid rows of its own z range (aligned to ``cz << 2`` = 16 planes) and nobody calls
    ``compute_multiscale``; the stores equal a one-rank two-pass run's at every level."""
    H, W, Z = 64, 96, 32
    chan = tmp_path / "data" / "Ex_488_Em_525"
    tiles = {"431040_368180": 0, "431040_394100": 1}
    for t, name in enumerate(tiles):
        a = MiniZarrArray.create(str(chan / (name + ".zarr") / "0"), (1, 1, Z, H, W), (1, 1, 4, 32, 32), np.uint16,
                                 compressor="zlib")  # fmt: skip
        a[0, 0] = synth.synthetic_stack(Z, H, W, n_unique=4) + np.uint16(t)
    d = tmp_path / "derivatives"
    d.mkdir()
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), np.full((H + 8, W + 8), 90, np.uint16))
    yy, xx = np.mgrid[0:H, 0:W]
    for side in (0, 1):
        f = (1.0 + 0.2 * side - 0.3 * ((yy - H / 2) / H) ** 2 - 0.2 * ((xx - W / 2) / W) ** 2).astype(np.float32)
        mini_tiff.imwrite(str(d / "flat_{}.tif".format(side)), f)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fused_rank_worker.py")
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DSX_RDZV_DIR", "DSX_FORCE_COMM")}

    def launch(world, results, mode):  # every process started once, each under its own time limit; no retry
        procs = []
        for r in range(world):
            env = dict(base, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT="29578", DSX_RDZV_DIR=str(tmp_path / ("rdzv_" + mode)))  # fmt: skip
            procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path), str(results), mode], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))  # fmt: skip
        outs = []
        try:
            for p in procs:
                so, se = p.communicate(timeout=300)
                assert p.returncode == 0, se[-3000:]
                outs.append(json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1]))
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        return sorted(outs, key=lambda o: o["rank"])

    one = launch(1, tmp_path / "r1", "two-pass")
    two = launch(2, tmp_path / "r2", "fused")
    names = [n + ".zarr" for n in tiles]
    assert one[0]["done"] == {n: Z for n in names} and one[0]["multiscale_calls"] == 2 and not one[0]["fused_pyramid"]
    assert [o["z_range"] for o in two] == [[0, 16], [16, 32]]
    assert all(o["z_range"][0] % (4 << 2) == 0 and o["z_range"][1] % (4 << 2) == 0 for o in two)
    assert all(o["multiscale_calls"] == 0 and o["fused_pyramid"] and o["pyramid_levels"] == [1, 2] for o in two)
    assert [o["done"] for o in two] == [{n: Z // 2 for n in names}] * 2
    for name in names:
        _assert_same_stores(str(tmp_path / "r1" / "destriped_data" / "Ex_488_Em_525" / name),
                            str(tmp_path / "r2" / "destriped_data" / "Ex_488_Em_525" / name), 3)  # fmt: skip


def _corrupt(path):
    """Set the reserved bit of the first Blosc block's zstd frame header."""
    with open(path, "rb") as fh:
        frame = bytearray(fh.read())
    pos = struct.unpack("<I", frame[16:20])[0] + 4
    assert frame[pos : pos + 4] == b"\x28\xb5\x2f\xfd"
    frame[pos + 4] |= 0x08
    with open(path, "wb") as fh:
        fh.write(bytes(frame))


def test_corrupted_chunk_with_fused_pyramid_raises_naming_it_and_a_good_run_follows(tmp_path):
    in_path, src = _make_input(tmp_path, 128, 256, 256)
    files = sorted(os.path.join(d, f) for d, _, fs in os.walk(src.path) for f in fs if not f.startswith("."))
    victim = files[2]
    with open(victim, "rb") as fh:
        good = fh.read()
    _corrupt(victim)
    g = str(tmp_path / "g")
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0, device_retile=True,
              device_decode=True, pyramid_group=g, n_levels=3)  # fmt: skip
    try:
        with pytest.raises(ValueError) as ei:
            zd.destripe_zarr_store(in_path, os.path.join(g, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None, **kw)
        want = os.path.join(os.path.basename(src.path.rstrip(os.sep)), os.path.relpath(victim, src.path)) + ")"
        assert want in str(ei.value), (want, str(ei.value))
        zd.release_staging()
        with open(victim, "wb") as fh:
            fh.write(good)
        n, _ = zd.destripe_zarr_store(in_path, os.path.join(g, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None, **kw)
        assert n == 128
        pyr = fo.pyramid(MiniZarrArray.open(os.path.join(g, "0"))[0, 0], 3)
        for lvl in (1, 2):
            assert np.array_equal(MiniZarrArray.open(os.path.join(g, str(lvl)))[0, 0], pyr[lvl]), lvl
    finally:
        zd.release_staging()
