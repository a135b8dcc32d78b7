"""``device_decode="full"`` on the GPU: Blosc chunks with zlib or blosclz inside and the chunks of a plain-zlib store
decoded by ``k_zdec_all`` (``csrc/dsx_zdec_kernels.h`` with ``csrc/dsx_inflate.h``).  ``destripe_zarr_store`` on the
recoded stores writes the chunk files of the host-decode run over the same voxels stored as Blosc-zstd."""

import json
import os
import zlib

import numpy as np
import pytest

import blosc_any_frames as baf
import inflate_cases as ic
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import pyramid
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from test_gpu_device_decode import _chunk_files, _device_decode, _named, _same_store
from test_gpu_device_decode_any import BLOCK, _lz4_split, _make_zstd_input, _recoded_copy, _run

pytestmark = pytest.mark.gpu


def _zlib_frame(raw):
    return ic.blosc_frame(raw, BLOCK, ic.ZLIB, baf.SHUFFLE, split=True)


def _blosclz_frame(raw):
    return ic.blosc_frame(raw, BLOCK, baf.BLOSCLZ, baf.SHUFFLE, split=True, runs_only=True)


def _plain_zlib_copy(zstd_path, root):
    """The store recoded to the plain ``zlib`` compressor (level 1, what ``mini_zarr`` writes)."""
    path, _, files = _recoded_copy(zstd_path, root, lambda i, raw: zlib.compress(raw, 1))
    meta_path = os.path.join(path, ".zarray")
    with open(meta_path) as f:
        meta = json.load(f)
    meta["compressor"] = {"id": "zlib", "level": 1}
    with open(meta_path, "w") as f:
        json.dump(meta, f)
    src = MiniZarrArray.open(path)
    assert src.compressor[0] == "zlib"
    return path, src, files


def test_golden_frames_on_the_device(tmp_path):
    """The frames of the real c-blosc: the kernel returns what ``dsx_blosc_decode_ref`` returns, the payload."""
    e = eng_mod.DestripeEngine(0)
    try:
        for i, (name, frame, raw) in enumerate(ic.golden_all_frames()):
            p = str(tmp_path / "f{}".format(i))
            with open(p, "wb") as f:
                f.write(frame)
            packed, tasks, routes = eng_mod.io_read_frames([p], len(raw), mode=eng_mod.ZDEC_ALL)
            assert int(routes[0]) == eng_mod.ROUTE_DEVICE, name
            dev, dev_st = _device_decode(e, packed, tasks, len(raw))
            assert not dev_st.any(), (name, dev_st)
            assert dev.tobytes() == raw, name
    finally:
        e.close()


@pytest.mark.parametrize("codec", ["blosc-zlib", "blosc-blosclz", "zlib"])
def test_recoded_store(tmp_path, codec):
    """Every chunk on the device with ``"full"``; ``True`` keeps the Blosc stores on the host and refuses the plain-zlib
    one; the output is that of the host-decode run."""
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)
    if codec == "zlib":
        path, src, files = _plain_zlib_copy(zstd_path, str(tmp_path / "re"))
    else:
        fn = _zlib_frame if codec == "blosc-zlib" else _blosclz_frame
        path, src, files = _recoded_copy(zstd_path, str(tmp_path / "re"), lambda i, raw: fn(raw), codec.split("-")[1])
    try:
        want = str(tmp_path / "want.zarr")
        assert _run(zstd_path, want, H, W, device_decode=False) == 64
        got = str(tmp_path / "all.zarr")
        assert _run(path, got, H, W, device_decode="full") == 64
        assert zd.LAST_RUN["device_decode"] is True and zd.LAST_RUN["device_decode_mode"] == "full"
        assert zd.LAST_RUN["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
        _same_store(want, got)
        host = str(tmp_path / "true.zarr")
        if codec == "zlib":
            for mode in (True, "any"):
                with pytest.raises(ValueError, match="device_decode needs a Blosc uint16 input"):
                    _run(path, host, H, W, device_decode=mode)
            assert _run(path, host, H, W, device_decode=False) == 64  # the host reader of the plain-zlib store
        else:
            assert _run(path, host, H, W, device_decode=True) == 64
            assert zd.LAST_RUN["decode_routes"] == {"device": 0, "host": len(files), "fill": 0}
        _same_store(want, host)
    finally:
        zd.release_staging()


def test_all_gives_the_routes_and_bytes_of_any_on_a_zstd_lz4_store(tmp_path):
    H, W = 256, 512  # 8 chunks
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)

    def fn(i, raw):
        if i % 4 == 1:
            return _lz4_split(raw)
        if i % 4 == 2:
            return baf.blosc_frame(raw, BLOCK, baf.ZSTD, baf.BITSHUFFLE, split=True)
        if i == 4:
            return None
        if i == 7:
            return _zlib_frame(raw)  # (the host's with "any", the device's with "full")
        return baf.blosc_frame(raw, BLOCK, baf.ZSTD, baf.SHUFFLE, split=False)

    mixed, _, files = _recoded_copy(zstd_path, str(tmp_path / "mixed"), fn)
    try:
        a, b = str(tmp_path / "any.zarr"), str(tmp_path / "all.zarr")
        assert _run(mixed, a, H, W, device_decode="any") == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": 6, "host": 1, "fill": 1}
        assert _run(mixed, b, H, W, device_decode="full") == 64
        assert zd.LAST_RUN["decode_routes"] == {"device": 7, "host": 0, "fill": 1}
        _same_store(a, b)
    finally:
        zd.release_staging()


def _flip_until_zlib_rejects(stream):
    """A byte in the middle of the stream flipped so that ``zlib.decompress`` refuses it."""
    for at in range(len(stream) // 2, len(stream)):
        bad = stream[:at] + bytes([stream[at] ^ 0x55]) + stream[at + 1 :]
        try:
            zlib.decompress(bad)
        except zlib.error:
            return bad
    raise AssertionError("no flip is refused")


@pytest.mark.parametrize("codec", ["blosc-zlib", "zlib"])
def test_corrupt_zlib_chunk_raises_naming_it_and_a_clean_run_follows(tmp_path, codec):
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 64, H, W)
    if codec == "zlib":
        path, src, files = _plain_zlib_copy(zstd_path, str(tmp_path / "re"))
    else:
        path, src, files = _recoded_copy(zstd_path, str(tmp_path / "re"), lambda i, raw: _zlib_frame(raw), "zlib")
    victim = files[2]
    with open(victim, "rb") as fh:
        good = fh.read()
    if codec == "zlib":
        bad = _flip_until_zlib_rejects(good)
    else:  # the first stream of block 0: [16-byte header][block table][int32 length][stream]
        pos = int.from_bytes(good[16:20], "little")
        cs = int.from_bytes(good[pos : pos + 4], "little")
        bad = good[: pos + 4] + _flip_until_zlib_rejects(good[pos + 4 : pos + 4 + cs]) + good[pos + 4 + cs :]
    with open(victim, "wb") as fh:
        fh.write(bad)
    try:
        with pytest.raises(ValueError, match="bad zlib stream" if codec != "zlib" else "zlib: bad chunk") as ei:
            _run(path, str(tmp_path / "o.zarr"), H, W, device_decode="full")
        if codec == "zlib":
            assert os.path.relpath(victim, src.path) in str(ei.value), str(ei.value)
        else:
            _named(ei.value, src, victim)
        assert "device decode status" in str(ei.value)
        with open(victim, "wb") as fh:
            fh.write(good)
        want, got = str(tmp_path / "want.zarr"), str(tmp_path / "all.zarr")
        assert _run(path, got, H, W, device_decode="full") == 64  # the same engine, the same process
        assert _run(zstd_path, want, H, W, device_decode=False) == 64
        _same_store(want, got)
    finally:
        zd.release_staging()


def test_all_with_device_codec_runs_and_fused_pyramid(tmp_path):
    H = W = 256
    zstd_path, _ = _make_zstd_input(str(tmp_path / "zstd"), 128, H, W)
    z_path, _, files = _recoded_copy(zstd_path, str(tmp_path / "zl"), lambda i, raw: _zlib_frame(raw) if i % 2 else _blosclz_frame(raw))
    try:
        groups = {}
        for tag, path, dec in (("want", zstd_path, False), ("all", z_path, "full")):
            g = groups[tag] = str(tmp_path / tag)
            assert _run(path, os.path.join(g, "0"), H, W, device_decode=dec, device_codec="runs", pyramid_group=g,
                        n_levels=3) == 128  # fmt: skip
            assert zd.LAST_RUN["fused_pyramid"] is True and zd.LAST_RUN["device_codec_mode"] == "runs"
        assert zd.LAST_RUN["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
        for lvl in range(3):
            _same_store(os.path.join(groups["want"], str(lvl)), os.path.join(groups["all"], str(lvl)))
    finally:
        zd.release_staging()


@pytest.mark.parametrize("codec", ["blosc-zlib", "zlib"])
def test_pipelined_pyramid_with_all(tmp_path, codec):
    """``compute_multiscale(pipelined=True, device_decode="full")`` over a level 0 recoded to zlib: the levels of the run
    over the Blosc-zstd level 0 with the host decoding."""
    H = W = 256
    chunks = (1, 1, 64, 128, 128)
    groups = {}
    for tag in ("want", "all"):
        g = groups[tag] = str(tmp_path / tag)
        os.makedirs(g)
        zstd_path, _ = _make_zstd_input(os.path.join(g, "in"), 128, H, W)
        if tag == "all" and codec == "zlib":
            path, _, files = _plain_zlib_copy(zstd_path, os.path.join(g, "re"))
        elif tag == "all":
            path, _, files = _recoded_copy(zstd_path, os.path.join(g, "re"), lambda i, raw: _zlib_frame(raw), "zlib")
        else:
            path = zstd_path
        os.rename(path, os.path.join(g, "0"))
    for tag, dec in (("want", False), ("all", "full")):
        zd.compute_multiscale(os.path.join(groups[tag], "0"), groups[tag], [2, 2, 2], 1, None, "t", n_levels=3,
                              chunks=chunks, compressor="blosc", device=0, pipelined=True, device_decode=dec,
                              io_threads=8)  # fmt: skip
    assert pyramid.LAST_PYRAMID["decode_routes"] == {"device": len(files), "host": 0, "fill": 0}
    for lvl in (1, 2):
        _same_store(os.path.join(groups["want"], str(lvl)), os.path.join(groups["all"], str(lvl)))
