"""The runs mode of the device encoder on the GPU (``k_zenc_block_runs``, ``device_codec="runs"``): the device writes the
bytes of the host build (held to libzstd, c-blosc and the decoders by tests/test_zstd_encoder_runs_host.py); stores
written with it hold the voxels of the host-codec store in fewer bytes than ``device_codec=True``, read back through the
host reader and through the device decoder; the fused pyramid uses it too; ``device_codec=True`` writes what it wrote."""

import os

import numpy as np
import pytest
from test_gpu_device_codec import _chunk_files
from test_gpu_device_decode import _device_decode
from test_gpu_fused_pyramid import _assert_same_stores, _both_routes, _make_input
from test_zstd_encoder_host import _bricks
from test_zstd_encoder_runs_host import edge_cases, frame_blocks

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu


def _device_frames(e, chunks, clevel=3, mode="runs"):
    chunks = np.ascontiguousarray(chunks, np.uint16)
    n = chunks.shape[0]
    nb = chunks.nbytes // n
    d_src = e.alloc(max(chunks.nbytes, 2))
    d_frames = e.alloc(n * (nb + 16) + 1)
    d_off = e.alloc(8 * (n + 1))
    try:
        d_src.upload(chunks)
        e.blosc_encode_device(d_src, n, nb, d_frames, d_off, typesize=2, clevel=clevel, mode=mode)
        e.sync()
        offsets = d_off.download((n + 1,), np.int64)
        frames = d_frames.download((n * (nb + 16) + 1,), np.uint8)[: offsets[-1]].tobytes()
    finally:
        for b in (d_src, d_frames, d_off):
            b.free()
    return frames, offsets


def _decode_on_the_device(e, tmp_path, frames, off, chunks):
    """The frames as chunk files through dsx_io_read_frames and k_zdec: the device route for every frame, the chunks."""
    n, nbytes = chunks.shape[0], chunks.nbytes // chunks.shape[0]
    paths = [str(tmp_path / "chunk.{}".format(i)) for i in range(n)]
    for i, p in enumerate(paths):
        with open(p, "wb") as f:
            f.write(frames[off[i] : off[i + 1]])
    packed, tasks, routes = eng_mod.io_read_frames(paths, nbytes)
    assert np.all(routes[:n] == eng_mod.ROUTE_DEVICE)
    out, status = _device_decode(e, packed, tasks, chunks.nbytes)
    assert not status.any(), status
    assert out.tobytes() == chunks.tobytes()


def test_device_frames_are_the_host_builds_bytes(tmp_path):
    rs = np.random.RandomState(11)
    bricks = np.stack([synth.synthetic_plane(k, 256, 4096).reshape(64, 128, 128) for k in range(6)])
    cases = [("bricks(8)", _bricks(8)), ("bricks", bricks), ("zeros", np.zeros((3, 64, 64, 64), np.uint16)),
             ("noise", rs.randint(0, 65536, (3, 100000)).astype(np.uint16)),
             ("short", rs.randint(0, 3, (5, 40)).astype(np.uint16)),
             ("poisson", (rs.poisson(40, (4, 3 * 65536 + 1000)) + 0x300).astype(np.uint16))]  # fmt: skip
    fib = np.repeat(np.arange(24), [int(round(1.618 ** k)) for k in range(24)])[:131072]
    cases.append(("fibonacci", np.stack([np.resize(rs.permutation(fib), 131072), np.arange(131072) % 129]).astype(np.uint16) | 0x700))
    cases += edge_cases()
    e = eng_mod.DestripeEngine(0)
    try:
        with_sequences = 0
        for name, c in cases:
            ref_frames, ref_off = eng_mod.blosc_encode_ref(c, mode="runs")
            frames, off = _device_frames(e, c)
            assert np.array_equal(off, ref_off), name
            assert frames == ref_frames, name
            with_sequences += any(s for k in range(c.shape[0]) for _, _, s in frame_blocks(frames[off[k] : off[k + 1]]))
            for k in range(c.shape[0]):
                assert mini_zarr.blosc_decode(frames[off[k] : off[k + 1]], c[k].nbytes) == c[k].tobytes(), (name, k)
            _decode_on_the_device(e, tmp_path, frames, off, np.ascontiguousarray(c, np.uint16))
        assert with_sequences >= 8
        frames, off = _device_frames(e, bricks, clevel=0)
        assert frames == eng_mod.blosc_encode_ref(bricks, clevel=0, mode="runs")[0]
        # the other mode of the same entry point: the bytes of the entry point without a mode
        old = eng_mod.blosc_encode_ref(bricks)
        assert _device_frames(e, bricks, mode="literals")[0] == old[0]
        with pytest.raises(ValueError):
            _device_frames(e, bricks, mode="lz")
    finally:
        e.close()


def _stores(tmp_path, Z, H, W, sc=None, codecs=(False, True, "runs"), **kw):
    vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    src = MiniZarrArray.create(str(tmp_path / "X_0_Y_0.zarr"), (1, 1, Z, H, W), (1, 1, 64, 128, 128), np.uint16,
                               compressor="blosc")  # fmt: skip
    for z in range(0, Z, 64):
        src[0, 0, z : z + 64] = vol[z : z + 64]
    outs = {}
    for codec in codecs:
        path = str(tmp_path / "out_{}.zarr".format(codec))
        n, _ = zd.destripe_zarr_store(str(tmp_path / "X_0_Y_0.zarr"), path, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                      sc, prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128),
                                      device=0, device_retile=True, compressor="blosc", io_threads=16,
                                      device_codec=codec, **kw)  # fmt: skip
        assert n == Z
        assert zd.LAST_RUN["device_codec"] is bool(codec)
        assert zd.LAST_RUN["device_codec_mode"] == {False: None, True: "literals", "runs": "runs"}[codec]
        outs[codec] = MiniZarrArray.open(path)
    zd.release_staging()
    return outs


def _check_stores(outs, chunk_bytes):
    assert np.array_equal(outs["runs"][0, 0], outs[False][0, 0])
    files = _chunk_files(outs["runs"])
    old_files = _chunk_files(outs[True])
    assert [os.path.relpath(p, outs["runs"].path) for p in files] == [os.path.relpath(p, outs[True].path) for p in old_files]
    sizes, old_sizes = ([os.path.getsize(p) for p in fs] for fs in (files, old_files))
    assert all(a <= b for a, b in zip(sizes, old_sizes))
    assert sum(sizes) < sum(old_sizes)
    for p in files:  # every chunk file through the host reader
        with open(p, "rb") as f:
            assert len(mini_zarr.blosc_decode(f.read(), chunk_bytes)) == chunk_bytes
    return sum(sizes), sum(old_sizes), sum(os.path.getsize(p) for p in _chunk_files(outs[False]))


def _read_back_on_the_device(tmp_path, store, Z, H, W):
    """The store as the input of a second pass with device_decode on and off: the same voxels, and every chunk file
    is one the device decodes."""
    files = _chunk_files(store)
    assert np.all(eng_mod.io_read_frames(files, 64 * 128 * 128 * 2)[2] == eng_mod.ROUTE_DEVICE)
    got = {}
    for decode in (False, True):
        path = str(tmp_path / "again_{}.zarr".format(int(decode)))
        zd.destripe_zarr_store(store.path, path, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None, tile_name="X_0_Y_0",
                               prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128), device=0,
                               device_retile=True, compressor="blosc", io_threads=16, device_decode=decode)  # fmt: skip
        got[decode] = MiniZarrArray.open(path)[0, 0]
    zd.release_staging()
    assert np.array_equal(got[True], got[False])


def test_store_with_runs_2048(tmp_path):
    """128 planes of 2048^2 = two z blocks: both staging buffers and frame buffers are used."""
    outs = _stores(tmp_path, 128, 2048, 2048)
    runs, old, host = _check_stores(outs, 64 * 128 * 128 * 2)
    print("2048^2 x 128: runs", runs, "entropy-only", old, "host writer", host)
    _read_back_on_the_device(tmp_path, outs["runs"], 128, 2048, 2048)


def test_store_with_runs_production_tile(tmp_path):
    """1600 x 2000 (partial bricks at the y / x edges), 96 planes (a partial last z block), shading on."""
    H, W = 1600, 2000
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.15 * (((yy - H / 2.0) / (H / 2.0)) ** 2 + ((xx - W / 2.0) / (W / 2.0)) ** 2)).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": np.full((H, W), 100.0, np.float32)}
    outs = _stores(tmp_path, 96, H, W, sc)
    runs, old, host = _check_stores(outs, 64 * 128 * 128 * 2)
    print("1600 x 2000 x 96: runs", runs, "entropy-only", old, "host writer", host)
    _read_back_on_the_device(tmp_path, outs["runs"], 96, H, W)


def test_fused_pyramid_with_runs_equals_the_two_pass_route(tmp_path):
    """192 planes of 2048^2, three levels: the pyramid rows are encoded in runs mode too."""
    in_path, _ = _make_input(tmp_path, 192, 2048, 2048)
    try:
        a, b = _both_routes(tmp_path, in_path, "runs", 3, (64, 2048, 2048), (1, 1, 64, 128, 128), "blosc",
                            device_codec="runs", device_decode=True)  # fmt: skip
        assert zd.LAST_RUN["pyramid_levels"] == [1, 2] and zd.LAST_RUN["device_codec_mode"] == "runs"
        _assert_same_stores(a, b, 3)
        with_sequences = 0
        for lvl in (1, 2):  # every chunk file of the pyramid levels is the runs-mode frame of its voxels
            arr = MiniZarrArray.open(os.path.join(b, str(lvl)))
            for z in range(-(-arr.shape[2] // arr.chunks[2])):
                for y in range(-(-arr.shape[3] // arr.chunks[3])):
                    idx = (0, 0, z, y, 0)
                    with open(arr._chunk_path(idx), "rb") as f:
                        frame = f.read()
                    chunk = np.ascontiguousarray(arr._read_chunk(idx), np.uint16).reshape(1, -1)
                    assert frame == eng_mod.blosc_encode_ref(chunk, mode="runs")[0], (lvl, idx)
                    with_sequences += any(s for _, _, s in frame_blocks(frame))
        print("pyramid chunk files with sequences:", with_sequences)
        assert with_sequences > 0
    finally:
        zd.release_staging()


def test_other_strings_are_refused_and_true_writes_what_it_wrote(tmp_path):
    src = MiniZarrArray.create(str(tmp_path / "i.zarr"), (1, 1, 64, 256, 256), (1, 1, 64, 128, 128), np.uint16,
                               compressor="blosc")  # fmt: skip
    src[0, 0] = synth.synthetic_stack(64, 256, 256)
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0, compressor="blosc")
    with pytest.raises(ValueError):
        zd.destripe_zarr_store(str(tmp_path / "i.zarr"), str(tmp_path / "bad.zarr"), synth.CELLS_CONFIG,
                               synth.NO_CELLS_CONFIG, None, device_codec="lz", **kw)  # fmt: skip
    assert not os.path.exists(str(tmp_path / "bad.zarr"))
    zd.destripe_zarr_store(str(tmp_path / "i.zarr"), str(tmp_path / "o.zarr"), synth.CELLS_CONFIG,
                           synth.NO_CELLS_CONFIG, None, device_codec=True, **kw)  # fmt: skip
    zd.release_staging()
    out = MiniZarrArray.open(str(tmp_path / "o.zarr"))
    for y in range(2):
        for x in range(2):
            brick = np.ascontiguousarray(out[0, 0, :, 128 * y : 128 * y + 128, 128 * x : 128 * x + 128])
            with open(os.path.join(out.path, "0", "0", "0", str(y), str(x)), "rb") as f:
                assert f.read() == eng_mod.blosc_encode_ref(brick[None])[0], (y, x)
