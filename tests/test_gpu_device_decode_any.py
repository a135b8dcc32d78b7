"""``device_decode="any"`` on the GPU: LZ4, split-stream and bit-shuffled Blosc chunks decoded by ``k_zdec``
(``csrc/dsx_zdec_kernels.h`` with ``csrc/dsx_lz4_dec.h``): the same bytes and statuses as the host build of the decoder
on the corpus of tests/test_lz4_decoder_host.py, and ``destripe_zarr_store`` on LZ4 / mixed stores writes the chunk
files of the host-decode run over the same voxels stored as Blosc-zstd (the expected output never needs liblz4)."""

import json
import os
import shutil
import struct

import numpy as np
import pytest

import blosc_any_frames as baf
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from test_gpu_device_decode import _chunk_files, _device_decode, _named, _rewrite_chunks, _same_store
from test_lz4_decoder_host import _small_frames

pytestmark = pytest.mark.gpu

CHUNK = 64 * 128 * 128 * 2
BLOCK = 256 * 1024  # c-blosc's block size for these chunks at clevel 5


def _route_frames():
    raw = baf.brick(7, 65536)
    return [("{} {} {}".format(c, s, sp), baf.blosc_frame(raw, 32768, c, s, sp), raw)
            for c in (baf.LZ4, baf.ZSTD) for s in (baf.NOSHUFFLE, baf.SHUFFLE, baf.BITSHUFFLE) for sp in (True, False)]  # fmt: skip


def test_device_bytes_and_statuses_match_the_host_build(tmp_path):
    """Every frame of the CPU tests' corpus, then broken tasks: the kernel returns what dsx_blosc_decode_ref returns."""
    corpus = baf.hand_frames() + baf.golden_any_frames()[0] + _route_frames() + _small_frames()
    e = eng_mod.DestripeEngine(0)
    try:
        kinds = set()
        for i, (name, frame, raw) in enumerate(corpus):
            p = str(tmp_path / "f{}".format(i))
            with open(p, "wb") as f:
                f.write(frame)
            packed, tasks, routes = eng_mod.io_read_frames([p], len(raw), mode=eng_mod.ZDEC_ANY)
            assert int(routes[0]) == eng_mod.ROUTE_DEVICE, name
            ref, ref_st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
            dev, dev_st = _device_decode(e, packed, tasks, len(raw))
            assert not ref_st.any() and not dev_st.any(), (name, ref_st, dev_st)
            assert dev.tobytes() == raw and np.array_equal(dev, ref), name
            kinds |= set(int(k) for k in tasks["kind"])
        for c in (eng_mod.TASK_LZ4, eng_mod.TASK_ZSTD):
            for flags in (0, eng_mod.TASK_SHUFFLE, eng_mod.TASK_BITSHUFFLE):
                assert {c | flags, c | flags | eng_mod.TASK_SPLIT} <= kinds
        # malformed tasks (every class of them ran under the CPU sanitizers first): the same status words, no more
        good = baf.Lz4Asm().lit(b"abcdefgh").match(3, 20).lit(b"12345").end()[0]
        two = struct.pack("<I", len(good)) + good + struct.pack("<I", len(good)) + good
        long = bytearray(two)
        long[0:4] = struct.pack("<I", len(two))
        broken = [(good[:4], 33, eng_mod.TASK_LZ4), (good, 34, eng_mod.TASK_LZ4), (good, 32, eng_mod.TASK_LZ4),
                  (baf.lz4_sequence(b"abcdefgh", 9, 20) + baf.lz4_sequence(b"12345"), 33, eng_mod.TASK_LZ4),
                  (baf.lz4_sequence(b"abcdefgh", 3, 200) + baf.lz4_sequence(b"12345"), 33, eng_mod.TASK_LZ4),
                  (bytes([0xF0]) + b"\xff" * 40, 33, eng_mod.TASK_LZ4),
                  (bytes(long), 66, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT),
                  (two + b"\x00", 66, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT),
                  (two, 66, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT)]  # fmt: skip
        packed = np.frombuffer(b"".join(b for b, _, _ in broken), np.uint8)
        tasks = np.zeros(len(broken), eng_mod.TASK_DTYPE)
        at = 0
        for i, (b, want, kind) in enumerate(broken):
            tasks[i] = (at, 128 * i, len(b), want, kind, i)
            at += len(b)
        ref, ref_st = eng_mod.blosc_decode_ref(packed, tasks, 128 * len(broken))
        dev, dev_st = _device_decode(e, packed, tasks, 128 * len(broken))
        assert list(ref_st) == [1, 12, 12, 11, 12, 12, 1, 1, 0]
        assert list(dev_st) == list(ref_st)
    finally:
        e.close()


# ---- stores ------------------------------------------------------------------------------------------------------------
def _make_zstd_input(root, Z, H, W):
    os.makedirs(root)
    vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(4, H, W))
    path = os.path.join(root, "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, Z, H, W), (1, 1, 64, 128, 128), np.uint16, compressor="blosc")
    for z in range(0, Z, 64):
        src[0, 0, z : z + 64] = vol[z : z + 64]
    return path, src


def _recoded_copy(zstd_path, root, fn, cname=None):
    """The store copied under ``root`` (same tile name) with every chunk frame passed through ``fn(index, raw)``
    (``None`` removes the file); ``cname`` rewrites the compressor of ``.zarray``."""
    path = os.path.join(root, os.path.basename(zstd_path))
    shutil.copytree(zstd_path, path)
    src = MiniZarrArray.open(path)
    files = _chunk_files(src)
    index = {p: i for i, p in enumerate(files)}
    _rewrite_chunks(src, lambda p, frame: fn(index[p], mini_zarr.blosc_decode(frame, CHUNK)))
    if cname:
        meta_path = os.path.join(path, ".zarray")
        with open(meta_path) as f:
            meta = json.load(f)
        meta["compressor"]["cname"] = cname
        with open(meta_path, "w") as f:
            json.dump(meta, f)
    return path, MiniZarrArray.open(path), files


def _lz4_split(raw):
    return baf.blosc_frame(raw, BLOCK, baf.LZ4, baf.SHUFFLE, split=True)


def _run(in_path, out, H, W, **kw):
    n, _ = zd.destripe_zarr_store(in_path, out, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                  prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128), device=0,
                                  device_retile=True, compressor="blosc", io_threads=16, **kw)  # fmt: skip
    return n


def test_store_of_lz4_chunks(tmp_path):
    """numcodecs.Blosc()'s default layout: LZ4, byte shuffle, split blocks."""
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)
    lz4_path, src, files = _recoded_copy(zstd_path, str(tmp_path / "lz4"), lambda i, raw: _lz4_split(raw), "lz4")
    assert src.compressor[2] == "lz4" and all(open(p, "rb").read()[2] == (0x1 | (1 << 5)) for p in files)
    try:
        want = str(tmp_path / "want.zarr")
        assert _run(zstd_path, want, H, W, device_decode=False) == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": 0, "host": len(files), "fill": 0}
        got = str(tmp_path / "any.zarr")
        assert _run(lz4_path, got, H, W, device_decode="any") == 64
        assert zd.LAST_RUN["device_decode"] is True and zd.LAST_RUN["device_decode_mode"] == "any"
        assert zd.LAST_RUN["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
        _same_store(want, got)
        # device_decode=True keeps the routes of before: every LZ4 chunk is the I/O threads'
        host = str(tmp_path / "true.zarr")
        if baf.have_liblz4():
            assert _run(lz4_path, host, H, W, device_decode=True) == 64
            assert zd.LAST_RUN["device_decode_mode"] == "zstd"
            assert zd.LAST_RUN["decode_routes"] == {"device": 0, "host": len(files), "fill": 0}
            _same_store(want, host)
        else:  # the host route cannot decode LZ4 here at all
            with pytest.raises(eng_mod.DsxError, match="liblz4"):
                _run(lz4_path, host, H, W, device_decode=True)
        # and "any" changes nothing for the zstd store
        again = str(tmp_path / "any_zstd.zarr")
        assert _run(zstd_path, again, H, W, device_decode="any") == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
        _same_store(want, again)
    finally:
        zd.release_staging()


def test_mixed_store(tmp_path):
    """zstd unsplit, LZ4 split, bit-shuffled (LZ4 and zstd), split zstd, one blosclz chunk, one missing chunk."""
    H, W = 256, 512  # 8 chunks
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)

    def fn(i, raw):
        if i == 1:
            return _lz4_split(raw)
        if i == 2:
            return baf.blosc_frame(raw, BLOCK, baf.LZ4, baf.BITSHUFFLE, split=True)
        if i == 3:
            return baf.blosclz_frame(raw)
        if i == 4:
            return None
        if i == 5:
            return baf.blosc_frame(raw, BLOCK, baf.ZSTD, baf.SHUFFLE, split=True)
        if i == 6:
            return baf.blosc_frame(raw, 128 * 1024, baf.ZSTD, baf.BITSHUFFLE, split=False)
        if i == 7:
            return baf.blosc_frame(raw, 64 * 1024, baf.LZ4, baf.NOSHUFFLE, split=False)
        return mini_zarr.blosc_encode(raw, 2, 3, True)  # chunk 0: what the writer here emits

    mixed_path, _, files = _recoded_copy(zstd_path, str(tmp_path / "mixed"), fn)
    assert len(files) == 8
    os.remove(_chunk_files(MiniZarrArray.open(zstd_path))[4])  # the expected run fills the same chunk
    try:
        want, got = str(tmp_path / "want.zarr"), str(tmp_path / "any.zarr")
        assert _run(zstd_path, want, H, W, device_decode=False) == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": 0, "host": 7, "fill": 1}
        assert _run(mixed_path, got, H, W, device_decode="any") == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": 6, "host": 1, "fill": 1}
        _same_store(want, got)
    finally:
        zd.release_staging()


def _corrupt_lz4(path):
    """Zero the offset of the first match of the first coded stream of block 0 (status kErrOffset; a mutation of the
    CPU run under the sanitizers, tests/test_lz4_decoder_host.py)."""
    with open(path, "rb") as fh:
        frame = bytearray(fh.read())
    blocksize = struct.unpack("<I", frame[8:12])[0]
    pos = struct.unpack("<I", frame[16:20])[0]
    for _ in range(2):
        cs = struct.unpack("<I", frame[pos : pos + 4])[0]
        if cs != blocksize // 2:
            break
        pos += 4 + cs
    else:
        raise AssertionError("block 0 has no coded stream")
    ip = pos + 4
    ll = frame[ip] >> 4
    ip += 1
    if ll == 15:
        while True:
            b = frame[ip]
            ip += 1
            ll += b
            if b != 255:
                break
    ip += ll
    assert ip + 2 < pos + 4 + cs
    frame[ip : ip + 2] = b"\x00\x00"
    with open(path, "wb") as fh:
        fh.write(bytes(frame))


def test_corrupt_lz4_chunk_raises_naming_it_and_a_clean_run_follows(tmp_path):
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)
    lz4_path, src, files = _recoded_copy(zstd_path, str(tmp_path / "lz4"), lambda i, raw: _lz4_split(raw), "lz4")
    victim = files[2]
    with open(victim, "rb") as fh:
        good = fh.read()
    _corrupt_lz4(victim)
    try:
        with pytest.raises(ValueError, match="bad lz4 stream") as ei:
            _run(lz4_path, str(tmp_path / "o.zarr"), H, W, device_decode="any")
        _named(ei.value, src, victim)
        assert "status 11" in str(ei.value)
        with open(victim, "wb") as fh:
            fh.write(good)
        want, got = str(tmp_path / "want.zarr"), str(tmp_path / "any.zarr")
        assert _run(lz4_path, got, H, W, device_decode="any") == 64  # the same engine, the same process
        assert _run(zstd_path, want, H, W, device_decode=False) == 64
        _same_store(want, got)
    finally:
        zd.release_staging()


def test_any_with_device_codec_runs_and_fused_pyramid(tmp_path):
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 128, H, W)
    lz4_path, _, files = _recoded_copy(zstd_path, str(tmp_path / "lz4"), lambda i, raw: _lz4_split(raw), "lz4")
    try:
        groups = {}
        for tag, path, dec in (("want", zstd_path, False), ("any", lz4_path, "any")):
            g = groups[tag] = str(tmp_path / tag)
            assert _run(path, os.path.join(g, "0"), H, W, device_decode=dec, device_codec="runs", pyramid_group=g,
                        n_levels=3) == 128  # fmt: skip
            assert zd.LAST_RUN["fused_pyramid"] is True and zd.LAST_RUN["device_codec_mode"] == "runs"
        assert zd.LAST_RUN["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
        for lvl in range(3):
            _same_store(os.path.join(groups["want"], str(lvl)), os.path.join(groups["any"], str(lvl)))
    finally:
        zd.release_staging()
