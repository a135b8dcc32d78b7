"""Blosc-zstd input chunks decoded on the device (``dsx_blosc_decode_device``, ``csrc/dsx_zdec_kernels.h``): the same
bytes as the host build of the decoder (``dsx_blosc_decode_ref``, held to libzstd by tests/test_zstd_decoder_host.py)
and as the host reader, and ``destripe_zarr_store(device_decode=True)`` writes the stores of the host-decode run.  The
kernel itself is held to libzstd's input too, on every zstd mode and task layout: tests/test_gpu_zdec_cases.py."""

import os
import struct

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from test_zstd_decoder_host import _zlib_inside, blosc_frame_cblosc_layout, blosc_frames_corpus, golden_frames

pytestmark = pytest.mark.gpu


def _device_decode(e, packed, tasks, out_bytes):
    n = len(tasks)
    bufs = [e.alloc(max(packed.nbytes, 1)), e.alloc(max(tasks.nbytes, 1)), e.alloc(max(out_bytes, 1)),
            e.alloc(4 * max(n, 1))]  # fmt: skip
    d_packed, d_tasks, d_out, d_status = bufs
    try:
        if packed.nbytes:
            d_packed.upload(packed)
        if n:
            d_tasks.upload(tasks.view(np.uint8))
        e.blosc_decode_device(d_packed, packed.nbytes, d_tasks, n, d_out, d_status, out_bytes=out_bytes)
        e.sync()
        out = d_out.download((out_bytes,), np.uint8) if out_bytes else np.zeros(0, np.uint8)
        status = d_status.download((n,), np.int32) if n else np.zeros(0, np.int32)
    finally:
        for b in bufs:
            b.free()
    return out, status


def _write_chunks(tmp_path, frames):
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / "c{:04d}".format(i))
        if f is not None:
            with open(p, "wb") as fh:
                fh.write(f)
        paths.append(p)
    return paths


def _check_group(e, tmp_path, frames, chunk_bytes, expect):
    paths = _write_chunks(tmp_path, frames)
    packed, tasks, _ = eng_mod.io_read_frames(paths, chunk_bytes, fill_value=0x1234)
    out_bytes = len(frames) * chunk_bytes
    ref, ref_st = eng_mod.blosc_decode_ref(packed, tasks, out_bytes)
    dev, dev_st = _device_decode(e, packed, tasks, out_bytes)
    assert not ref_st.any() and not dev_st.any(), (ref_st, dev_st)
    assert np.array_equal(dev, ref)
    for i, want in enumerate(expect):
        assert dev[i * chunk_bytes : (i + 1) * chunk_bytes].tobytes() == want, i


def test_device_bytes_match_the_host(tmp_path):
    e = eng_mod.DestripeEngine(0)
    try:
        for gi, (chunk_bytes, frames, raws) in enumerate(blosc_frames_corpus()):
            d = tmp_path / "g{}".format(gi)
            d.mkdir()
            fill = struct.pack("<H", 0x1234) * (chunk_bytes // 2)
            expect = [r if f is not None else fill for f, r in zip(frames, raws)]
            _check_group(e, d, frames, chunk_bytes, expect)
        for k, (frame, raw) in enumerate(golden_frames()):
            d = tmp_path / "golden{}".format(k)
            d.mkdir()
            _check_group(e, d, [frame], len(raw), [raw])
        plane = synth.synthetic_plane(5, 1024, 2048).tobytes()  # 4 MiB
        for bs in (32 * 1024, 128 * 1024, 1 << 20):  # c-blosc's layouts at clevel 1, 3, 9
            d = tmp_path / "cb{}".format(bs)
            d.mkdir()
            _check_group(e, d, [blosc_frame_cblosc_layout(plane, bs, 5)], len(plane), [plane])
    finally:
        e.close()


def _make_input(tmp_path, Z, H, W, name="X_0_Y_0.zarr"):
    vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    path = str(tmp_path / name)
    src = MiniZarrArray.create(path, (1, 1, Z, H, W), (1, 1, 64, 128, 128), np.uint16, compressor="blosc")
    for z in range(0, Z, 64):
        src[0, 0, z : z + 64] = vol[z : z + 64]
    return path, src


def _run_pair(tmp_path, in_path, H, W, sc=None, device_codec=False):
    outs = {}
    for dec in (False, True):
        path = str(tmp_path / "out_{}.zarr".format(int(dec)))
        zd.destripe_zarr_store(in_path, path, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, sc,
                               prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128), device=0,
                               device_retile=True, compressor="blosc", io_threads=16, device_codec=device_codec,
                               device_decode=dec)  # fmt: skip
        outs[dec] = path
    zd.release_staging()
    return outs


def _same_store(a, b):
    fa = sorted(os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs)
    fb = sorted(os.path.relpath(os.path.join(d, f), b) for d, _, fs in os.walk(b) for f in fs)
    assert fa == fb
    for f in fa:
        with open(os.path.join(a, f), "rb") as x, open(os.path.join(b, f), "rb") as y:
            assert x.read() == y.read(), f


def test_store_device_decode_2048(tmp_path):
    """128 planes of 2048^2: two z blocks, both staging buffers."""
    in_path, _ = _make_input(tmp_path, 128, 2048, 2048)
    outs = _run_pair(tmp_path, in_path, 2048, 2048)
    _same_store(outs[False], outs[True])
    assert zd.LAST_RUN["device_decode"] is True


def test_store_device_decode_production_tile_with_device_codec(tmp_path):
    """1600 x 2000 (partial bricks), 96 planes (a partial last z block), shading on, device codec on."""
    H, W = 1600, 2000
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.15 * (((yy - H / 2.0) / (H / 2.0)) ** 2 + ((xx - W / 2.0) / (W / 2.0)) ** 2)).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": np.full((H, W), 100.0, np.float32)}
    in_path, _ = _make_input(tmp_path, 96, H, W)
    outs = _run_pair(tmp_path, in_path, H, W, sc, device_codec=True)
    _same_store(outs[False], outs[True])


def _rewrite_chunks(src, fn):
    for d, _, fs in os.walk(src.path):
        for f in fs:
            if f.startswith("."):
                continue
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                frame = fh.read()
            new = fn(p, frame)
            if new is None:
                os.remove(p)
            else:
                with open(p, "wb") as fh:
                    fh.write(new)


def test_store_device_decode_cblosc_layout_missing_and_zlib_chunks(tmp_path):
    """Chunks re-written in c-blosc's clevel-3 layout (128 KiB zstd blocks), some files missing, one zlib-inside frame
    (host route)."""
    in_path, src = _make_input(tmp_path, 64, 512, 512)
    nbytes = 64 * 128 * 128 * 2
    count = [0]

    def fn(p, frame):
        raw = mini_zarr.blosc_decode(frame, nbytes)
        count[0] += 1
        if count[0] in (3, 7):
            return None
        if count[0] == 5:
            return _zlib_inside(raw)
        return blosc_frame_cblosc_layout(raw, 128 * 1024, 5)

    _rewrite_chunks(src, fn)
    outs = _run_pair(tmp_path, in_path, 512, 512)
    _same_store(outs[False], outs[True])


def _chunk_files(src):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(src.path) for f in fs if not f.startswith("."))


def _corrupt(path):
    """Set the reserved bit of the first Blosc block's zstd frame header (a mutation the CPU sanitizer run covers)."""
    with open(path, "rb") as fh:
        frame = bytearray(fh.read())
    pos = struct.unpack("<I", frame[16:20])[0] + 4
    assert frame[pos : pos + 4] == b"\x28\xb5\x2f\xfd"
    frame[pos + 4] |= 0x08
    with open(path, "wb") as fh:
        fh.write(bytes(frame))


def _named(err, src, victim):
    """The error names exactly that chunk file: '<store>/<chunk key>)' ends the path in the message."""
    want = os.path.join(os.path.basename(src.path.rstrip(os.sep)), os.path.relpath(victim, src.path)) + ")"
    assert want in str(err), (want, str(err))


def test_corrupted_chunk_raises_naming_it(tmp_path):
    in_path, src = _make_input(tmp_path, 64, 256, 256)
    victim = _chunk_files(src)[2]
    _corrupt(victim)
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0, device_retile=True)
    with pytest.raises(ValueError) as ei:
        zd.destripe_zarr_store(in_path, str(tmp_path / "o.zarr"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                               device_decode=True, **kw)  # fmt: skip
    _named(ei.value, src, victim)
    zd.release_staging()


def test_corrupted_chunk_in_the_first_of_three_blocks(tmp_path):
    """Three z blocks: block 0's statuses are checked after the read of block 2 has refilled the same staging buffer.
    Block 2's chunks are missing (one fill task each), so it has fewer tasks than block 0."""
    in_path, src = _make_input(tmp_path, 192, 256, 256)
    files = _chunk_files(src)
    zkey = lambda p: os.path.relpath(p, src.path).split(os.sep)[2]  # noqa: E731  (t / c / z / y / x)
    for p in files:
        if zkey(p) == "2":
            os.remove(p)
    victim = [p for p in files if zkey(p) == "0"][-1]
    _corrupt(victim)
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0, device_retile=True)
    with pytest.raises(ValueError) as ei:
        zd.destripe_zarr_store(in_path, str(tmp_path / "o.zarr"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                               device_decode=True, **kw)  # fmt: skip
    _named(ei.value, src, victim)
    zd.release_staging()


def test_device_decode_needs_blosc_input_on_the_device_path(tmp_path):
    kw = dict(prediction_chunksize=(64, 256, 256), output_chunks=(1, 1, 64, 128, 128), device=0)
    for comp in (None, "zlib"):
        p = str(tmp_path / "i_{}.zarr".format(comp))
        src = MiniZarrArray.create(p, (1, 1, 64, 256, 256), (1, 1, 64, 128, 128), np.uint16, compressor=comp)
        src[0, 0] = synth.synthetic_stack(64, 256, 256)
        with pytest.raises(ValueError):
            zd.destripe_zarr_store(p, str(tmp_path / "o.zarr"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                   device_decode=True, **kw)  # fmt: skip
    p, _ = _make_input(tmp_path, 64, 256, 256, name="b.zarr")
    with pytest.raises(ValueError):
        zd.destripe_zarr_store(p, str(tmp_path / "o.zarr"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                               device_decode=True, device_retile=False, **kw)  # fmt: skip
