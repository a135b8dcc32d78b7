"""Blosc-zstd frames encoded on the device (``dsx_blosc_encode_device``, ``csrc/dsx_zenc_kernels.h``): byte-identical to
the host build of the encoder (``dsx_blosc_encode_ref``, itself held to libzstd / c-blosc by
tests/test_zstd_encoder_host.py), and ``destripe_zarr_store(device_codec=True)`` writes stores whose voxels are the
host-codec run's."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu


def _device_frames(e, chunks, clevel=3):
    chunks = np.ascontiguousarray(chunks, np.uint16)
    n = chunks.shape[0]
    nb = chunks.nbytes // n
    d_src = e.alloc(max(chunks.nbytes, 2))
    d_frames = e.alloc(n * (nb + 16) + 1)
    d_off = e.alloc(8 * (n + 1))
    try:
        if chunks.nbytes:
            d_src.upload(chunks)
        e.blosc_encode_device(d_src, n, nb, d_frames, d_off, typesize=2, clevel=clevel)
        e.sync()
        offsets = d_off.download((n + 1,), np.int64)
        frames = d_frames.download((n * (nb + 16) + 1,), np.uint8)[: offsets[-1]].tobytes()
    finally:
        for b in (d_src, d_frames, d_off):
            b.free()
    return frames, offsets


def test_device_frames_are_the_host_builds_bytes():
    rs = np.random.RandomState(11)
    bricks = np.stack([synth.synthetic_plane(k, 256, 4096).reshape(64, 128, 128) for k in range(6)])
    cases = [bricks, np.zeros((3, 64, 64, 64), np.uint16), rs.randint(0, 65536, (3, 100000)).astype(np.uint16),
             rs.randint(0, 3, (5, 40)).astype(np.uint16),
             (rs.poisson(40, (4, 3 * 65536 + 1000)) + 0x300).astype(np.uint16)]
    fib = np.repeat(np.arange(24), [int(round(1.618 ** k)) for k in range(24)])[:131072]
    cases.append(np.stack([np.resize(rs.permutation(fib), 131072), np.arange(131072) % 129]).astype(np.uint16) | 0x700)
    e = eng_mod.DestripeEngine(0)
    try:
        for i, c in enumerate(cases):
            ref_frames, ref_off = eng_mod.blosc_encode_ref(c)
            frames, off = _device_frames(e, c)
            assert np.array_equal(off, ref_off), i
            assert frames == ref_frames, i
            for k in range(c.shape[0]):
                assert mini_zarr.blosc_decode(frames[off[k] : off[k + 1]], c[k].nbytes) == c[k].tobytes(), (i, k)
        frames, off = _device_frames(e, bricks, clevel=0)
        assert frames == eng_mod.blosc_encode_ref(bricks, clevel=0)[0]
    finally:
        e.close()


def _store_pair(tmp_path, Z, H, W, sc=None):
    vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    src = MiniZarrArray.create(str(tmp_path / "X_0_Y_0.zarr"), (1, 1, Z, H, W), (1, 1, 64, 128, 128), np.uint16,
                               compressor="blosc")  # fmt: skip
    for z in range(0, Z, 64):
        src[0, 0, z : z + 64] = vol[z : z + 64]
    outs = {}
    for codec in (False, True):
        path = str(tmp_path / "out_{}.zarr".format(int(codec)))
        n, _ = zd.destripe_zarr_store(str(tmp_path / "X_0_Y_0.zarr"), path, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                      sc, prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128),
                                      device=0, device_retile=True, compressor="blosc", io_threads=16,
                                      device_codec=codec)  # fmt: skip
        assert n == Z
        outs[codec] = MiniZarrArray.open(path)
    zd.release_staging()
    return outs


def _chunk_files(arr):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(arr.path) for f in fs if not f.startswith("."))


def test_store_with_device_codec_equals_host_codec_2048(tmp_path):
    """128 planes of 2048^2 = two z blocks: both staging buffers and frame buffers are used."""
    outs = _store_pair(tmp_path, 128, 2048, 2048)
    assert np.array_equal(outs[True][0, 0], outs[False][0, 0])
    files = _chunk_files(outs[True])
    assert len(files) == 2 * 16 * 16
    dev_bytes = sum(os.path.getsize(p) for p in files)
    host_bytes = sum(os.path.getsize(p) for p in _chunk_files(outs[False]))
    assert dev_bytes <= 1.25 * host_bytes, (dev_bytes, host_bytes)
    for p in files[:: 37]:  # through the native reader directly, too
        with open(p, "rb") as f:
            frame = f.read()
        assert len(mini_zarr.blosc_decode(frame, 64 * 128 * 128 * 2)) == 64 * 128 * 128 * 2


def test_store_with_device_codec_equals_host_codec_production_tile(tmp_path):
    """1600 x 2000 (partial bricks at the y / x edges), 96 planes (a partial last z block), shading on."""
    H, W = 1600, 2000
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.15 * (((yy - H / 2.0) / (H / 2.0)) ** 2 + ((xx - W / 2.0) / (W / 2.0)) ** 2)).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": np.full((H, W), 100.0, np.float32)}
    outs = _store_pair(tmp_path, 96, H, W, sc)
    assert np.array_equal(outs[True][0, 0], outs[False][0, 0])


def test_device_codec_needs_blosc_zstd_on_the_device_path(tmp_path):
    src = MiniZarrArray.create(str(tmp_path / "i.zarr"), (1, 1, 64, 256, 256), (1, 1, 64, 128, 128), np.uint16)
    src[0, 0] = synth.synthetic_stack(64, 256, 256)
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0)
    for bad in (dict(compressor=None), dict(compressor="zlib"), dict(compressor="blosc", device_retile=False)):
        with pytest.raises(ValueError):
            zd.destripe_zarr_store(str(tmp_path / "i.zarr"), str(tmp_path / "o.zarr"), synth.CELLS_CONFIG,
                                   synth.NO_CELLS_CONFIG, None, device_codec=True, **kw, **bad)  # fmt: skip
