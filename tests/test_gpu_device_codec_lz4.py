"""The Blosc-LZ4 encoder on the GPU (``k_lz4_stream``, mode ``"lz4"`` of ``dsx_blosc_encode_device_ex``): the device
writes the bytes of the host build (held to liblz4, c-blosc and the decoders by tests/test_lz4_encoder_host.py) for the
whole case table of tests/lz4_enc_cases.py; a Blosc-LZ4 output store is the same set of files with the host writer and
with ``device_codec=True``, holds the voxels of the Blosc-zstd store, and is read back by the device decoder; the
pyramid levels of such an output go through the same encoder."""

import os

import lz4_enc_cases as lc
import numpy as np
import pytest
from test_gpu_device_decode import _device_decode

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import pyramid, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

LZ4_CONFIG = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


def _device_frames(e, chunks, clevel=5, mode="lz4"):
    chunks = np.ascontiguousarray(chunks, np.uint16)
    n = chunks.shape[0]
    nb = chunks.nbytes // n
    d_src = e.alloc(max(chunks.nbytes, 2))
    d_frames = e.alloc(n * (nb + 16) + 1)
    d_off = e.alloc(8 * (n + 1))
    try:
        if chunks.nbytes:
            d_src.upload(chunks)
        e.blosc_encode_device(d_src, n, nb, d_frames, d_off, typesize=2, clevel=clevel, mode=mode)
        e.sync()
        offsets = d_off.download((n + 1,), np.int64)
        frames = d_frames.download((n * (nb + 16) + 1,), np.uint8)[: offsets[-1]].tobytes()
    finally:
        for b in (d_src, d_frames, d_off):
            b.free()
    return frames, offsets


def test_device_frames_are_the_host_builds_bytes(tmp_path):
    """The whole case table, one launch per chunk size; then the frames as chunk files through dsx_io_read_frames in
    DSX_ZDEC_ANY mode and k_zdec; clevel 0; the two zstd modes of the same engine keep their bytes."""
    table = lc.cases() + [("image bricks", lc.image_bricks())]
    e = eng_mod.DestripeEngine(0)
    try:
        for k, (name, chunks) in enumerate(table):
            ref_frames, ref_off = eng_mod.blosc_encode_ref(chunks, clevel=5, mode="lz4")
            frames, off = _device_frames(e, chunks)
            assert np.array_equal(off, ref_off), name
            assert frames == ref_frames, name
            n, nbytes = chunks.shape[0], chunks.nbytes // chunks.shape[0]
            if not nbytes:
                continue
            paths = [str(tmp_path / "c{}.{}".format(k, i)) for i in range(n)]
            for i, p in enumerate(paths):
                with open(p, "wb") as f:
                    f.write(frames[off[i] : off[i + 1]])
            packed, tasks, routes = eng_mod.io_read_frames(paths, nbytes, mode=eng_mod.ZDEC_ANY)
            assert np.all(routes[:n] == eng_mod.ROUTE_DEVICE), name
            out, status = _device_decode(e, packed, tasks, chunks.nbytes)
            assert not status.any(), (name, status)
            assert out.tobytes() == chunks.tobytes(), name
        bricks = table[-1][1]
        frames, off = _device_frames(e, bricks, clevel=0)
        want = eng_mod.blosc_encode_ref(bricks, clevel=0, mode="lz4")
        assert frames == want[0] and np.array_equal(off, want[1]) and frames[2] & lc.MEMCPYED
        for mode in ("literals", "runs"):
            assert _device_frames(e, bricks, clevel=3, mode=mode)[0] == eng_mod.blosc_encode_ref(bricks, mode=mode)[0], mode
        with pytest.raises(ValueError):
            _device_frames(e, bricks, mode="lz")
    finally:
        e.close()


def _chunk_files(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs if not f.startswith("."))


def _assert_same_files(a, b):
    assert _chunk_files(a) == _chunk_files(b) and _chunk_files(a)
    for f in _chunk_files(a):
        with open(os.path.join(a, f), "rb") as fa, open(os.path.join(b, f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_lz4_output_store_both_routes_then_read_back_then_a_zstd_output(tmp_path):
    Z, H, W = 64, 256, 256
    src = MiniZarrArray.create(str(tmp_path / "X_0_Y_0.zarr"), (1, 1, Z, H, W), (1, 1, 64, 128, 128), np.uint16,
                               compressor="blosc")  # fmt: skip
    src[0, 0] = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    kw = dict(prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128), device=0, device_retile=True, io_threads=8)

    def run(tag, compressor, codec, source=src.path, **more):
        path = str(tmp_path / tag)
        n, _ = zd.destripe_zarr_store(source, path, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None, tile_name="X_0_Y_0",
                                      compressor=compressor, device_codec=codec, **kw, **more)  # fmt: skip
        assert n == Z
        return path

    try:
        with pytest.raises(ValueError):
            run("refused", LZ4_CONFIG, "runs")
        assert not os.path.exists(str(tmp_path / "refused"))
        host = run("lz4_host", LZ4_CONFIG, False)
        assert zd.LAST_RUN["device_codec"] is False and zd.LAST_RUN["device_codec_mode"] is None
        dev = run("lz4_device", LZ4_CONFIG, True)
        assert zd.LAST_RUN["device_codec"] is True and zd.LAST_RUN["device_codec_mode"] == "lz4"
        # a zstd output of the same geometry in the same process: staging buffers of the LZ4 run must not serve it
        zstd_dev = run("zstd_device", "blosc", True)
        assert zd.LAST_RUN["device_codec_mode"] == "literals"
        zstd_host = run("zstd_host", "blosc", False)
        _assert_same_files(host, dev)
        voxels = MiniZarrArray.open(zstd_host)[0, 0]
        assert np.array_equal(MiniZarrArray.open(dev)[0, 0], voxels)
        assert np.array_equal(MiniZarrArray.open(zstd_dev)[0, 0], voxels)
        out = MiniZarrArray.open(dev)
        for y in range(2):
            for x in range(2):  # the files are the encoder's frames of their voxels, and zstd frames where zstd was asked for
                brick = np.ascontiguousarray(voxels[:, 128 * y : 128 * y + 128, 128 * x : 128 * x + 128]).reshape(1, -1)
                with open(out._chunk_path((0, 0, 0, y, x)), "rb") as f:
                    assert f.read() == eng_mod.blosc_encode_ref(brick, clevel=5, mode="lz4")[0], (y, x)
                with open(MiniZarrArray.open(zstd_dev)._chunk_path((0, 0, 0, y, x)), "rb") as f:
                    assert f.read() == eng_mod.blosc_encode_ref(brick, clevel=3)[0], (y, x)
        # the LZ4 store as the input of a second pass, decoded on the device
        files = [os.path.join(dev, f) for f in _chunk_files(dev)]
        assert np.all(eng_mod.io_read_frames(files, 64 * 128 * 128 * 2, mode=eng_mod.ZDEC_ANY)[2] == eng_mod.ROUTE_DEVICE)
        again = {}
        for decode in (False, "any"):
            again[decode] = run("again_{}".format(decode), "blosc", False, source=dev, device_decode=decode)
            if decode:
                assert zd.LAST_RUN["decode_routes"] == {"device": 4, "host": 0, "fill": 0}
        assert np.array_equal(MiniZarrArray.open(again["any"])[0, 0], MiniZarrArray.open(again[False])[0, 0])
    finally:
        zd.release_staging()


def test_fused_pyramid_levels_of_an_lz4_output(tmp_path):
    """24 x 64 x 96 in chunks (4, 32, 32), three levels: the levels written by the device LZ4 encoder are the files of
    the host route."""
    Z, H, W = 24, 64, 96
    chunks = (1, 1, 4, 32, 32)
    src = MiniZarrArray.create(str(tmp_path / "X_0_Y_0.zarr"), (1, 1, Z, H, W), chunks, np.uint16, compressor="blosc")
    src[0, 0] = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    groups = {}
    try:
        for codec in (False, True):
            g = groups[codec] = str(tmp_path / "fused_{}".format(int(codec)))
            n, _ = zd.destripe_zarr_store(src.path, os.path.join(g, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                          prediction_chunksize=(4, H, W), output_chunks=chunks, device=0, device_retile=True,
                                          compressor=LZ4_CONFIG, io_threads=8, device_codec=codec, pyramid_group=g,
                                          n_levels=3)  # fmt: skip
            assert n == Z and zd.LAST_RUN["fused_pyramid"] is True and zd.LAST_RUN["pyramid_levels"] == [1, 2]
            assert zd.LAST_RUN["device_codec_mode"] == ("lz4" if codec else None)
        for lvl in range(3):
            a, b = (os.path.join(groups[c], str(lvl)) for c in (False, True))
            assert MiniZarrArray.open(b).compressor_meta == LZ4_CONFIG
            _assert_same_files(a, b)
            assert np.array_equal(MiniZarrArray.open(a)[0, 0], MiniZarrArray.open(b)[0, 0]), lvl
    finally:
        zd.release_staging()


def test_pipelined_pyramid_of_an_lz4_group(tmp_path):
    """150 x 203 x 301 in chunks (16, 32, 32), four levels, from a Blosc-LZ4 level 0: the slab route (host writer), the
    pipelined route with the host writer, and with the device encoder and decoder."""
    from oracle import format_oracle as fo

    rs = np.random.RandomState(7)
    vol = synth.synthetic_stack(150, 203, 301, n_unique=4).astype(np.uint16)
    vol[:, :70, :100] = 0x1200 + rs.randint(0, 256, (150, 70, 100))
    chunks = (1, 1, 16, 32, 32)
    groups = {}
    for tag, kw in (("slabs", {}), ("host", dict(pipelined=True, io_threads=8)),
                    ("device", dict(pipelined=True, io_threads=8, device_codec=True, device_decode="any"))):  # fmt: skip
        g = groups[tag] = str(tmp_path / tag)
        a = MiniZarrArray.create(os.path.join(g, "0"), (1, 1) + vol.shape, chunks, np.uint16, compressor=LZ4_CONFIG)
        a[0, 0] = vol
        zd.compute_multiscale(os.path.join(g, "0"), g, [2, 2, 2], 1, None, "t", n_levels=4, chunks=chunks,
                              compressor=LZ4_CONFIG, device=0, **kw)  # fmt: skip
        assert pyramid.LAST_PYRAMID["route"] == ("slabs" if tag == "slabs" else "pipelined")
        if tag == "device":
            routes = pyramid.LAST_PYRAMID["decode_routes"]
            assert routes["host"] == 0 and routes["fill"] == 0 and routes["device"] > 0
    with pytest.raises(ValueError):
        zd.compute_multiscale(os.path.join(groups["host"], "0"), str(tmp_path / "refused"), [2, 2, 2], 1, None, "t",
                              n_levels=4, chunks=chunks, compressor=LZ4_CONFIG, device=0, pipelined=True, device_codec="runs")  # fmt: skip
    want = fo.pyramid(vol, 4)
    for lvl in range(1, 4):
        paths = [os.path.join(groups[t], str(lvl)) for t in ("slabs", "host", "device")]
        assert MiniZarrArray.open(paths[2]).compressor_meta == LZ4_CONFIG
        _assert_same_files(paths[0], paths[1])
        _assert_same_files(paths[1], paths[2])
        assert np.array_equal(MiniZarrArray.open(paths[2])[0, 0], want[lvl]), lvl
