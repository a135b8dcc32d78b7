"""The digest manifest of an array (``mini_zarr.MiniZarrArray.create(digests=True)``) and reading a store back against it
on the host build (``integrity.verify_store(device=None)``), on a 22 x 70 x 100 volume in chunks of (4, 32, 32): a ragged
last chunk on every axis.  No GPU needed."""

import json
import os
import shutil

import numpy as np
import pytest

import digest_cases as dc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import integrity
from aind_smartspim_destripe_amd.mini_zarr import DIGEST_BIN, DIGEST_JSON, MiniZarrArray

ZYX, CHUNKS = (22, 70, 100), (1, 1, 4, 32, 32)
SHAPE = (1, 1) + ZYX
GRID = (6, 3, 4)
LZ4 = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


def _volume(seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, ZYX, dtype=np.uint16)


def _smooth_volume():
    """Compressible voxels (so that a Blosc chunk is really compressed), no chunk equal to another or to the fill."""
    z, y, x = np.meshgrid(*[np.arange(n) for n in ZYX], indexing="ij")
    return (1000 + 37 * z + 5 * y + x // 3).astype(np.uint16)


def _write(path, vol, compressor=None, **kw):
    arr = MiniZarrArray.create(str(path), SHAPE, CHUNKS, np.uint16, compressor=compressor, digests=True, **kw)
    arr[0, 0] = vol
    return arr


def _readback_records(arr):
    """The restatement of the chunks as the host decoders read them back."""
    return dc.restate_array(arr[0, 0], CHUNKS[-3:])


def _chunk_file(arr, n):
    g = np.unravel_index(n, GRID)
    return arr._chunk_path((0, 0) + tuple(int(i) for i in g))


def test_manifest_files_and_slab_writes(tmp_path):
    vol = _volume()
    arr = MiniZarrArray.create(str(tmp_path / "a"), SHAPE, CHUNKS, np.uint16, digests=True)
    assert arr.digest_grid == GRID
    with open(tmp_path / "a" / DIGEST_JSON) as f:
        man = json.load(f)
    assert man == {"format": 1, "algorithm": "dsx-sm64-rowcol", "shape": list(SHAPE), "chunks": list(CHUNKS),
                   "dtype": "<u2", "fill_value": 0, "grid": list(GRID)}  # fmt: skip
    assert os.path.getsize(tmp_path / "a" / DIGEST_BIN) == 72 * 24
    rec = arr.digest_records()
    assert rec.dtype == eng_mod.DIGEST_DTYPE and rec.shape == (72,) and not rec["count"].any()  # nothing recorded yet
    for z in range(0, 22, 8):  # slabs of two chunk rows
        arr[0, 0, z : z + 8] = vol[z : z + 8]
    assert dc.as_triples(arr.digest_records()) == dc.restate_array(vol, CHUNKS[-3:]) == _readback_records(arr)
    # partial chunks: a box that cuts chunks on every axis goes through the read-modify-write
    vol[3:11, 30:41, 90:100] = 7
    arr[0, 0, 3:11, 30:41, 90:100] = 7
    vol[21, 69, 99] = 65535
    arr[0, 0, 21, 69, 99] = 65535
    assert np.array_equal(arr[0, 0], vol)
    assert dc.as_triples(arr.digest_records()) == dc.restate_array(vol, CHUNKS[-3:])
    # a whole brick in chunk order, its padding filled with something: the padding never enters
    brick = np.full(CHUNKS[-3:], 0xBEEF, np.uint16)
    brick[:2, :6, :4] = vol[20:22, 64:70, 96:100] = 123
    arr.write_chunk_flat((0, 0, 5, 2, 3), brick.reshape(-1))
    assert dc.as_triples(arr.digest_records()) == dc.restate_array(vol, CHUNKS[-3:])
    reopened = MiniZarrArray.open(str(tmp_path / "a"))
    assert reopened.digest_grid == GRID and np.array_equal(reopened.digest_records(), arr.digest_records())


@pytest.mark.parametrize("compressor", [None, "zlib", "blosc", LZ4], ids=["raw", "zlib", "blosc-zstd", "blosc-lz4"])
def test_records_do_not_depend_on_the_codec_and_chunk_files_do_not_change(tmp_path, compressor):
    vol = _smooth_volume()
    with_m = _write(tmp_path / "with", vol, compressor)
    plain = MiniZarrArray.create(str(tmp_path / "plain"), SHAPE, CHUNKS, np.uint16, compressor=compressor)
    plain[0, 0] = vol
    assert dc.as_triples(with_m.digest_records()) == dc.restate_array(vol, CHUNKS[-3:])
    names = lambda p: sorted(os.path.relpath(os.path.join(d, f), p) for d, _, fs in os.walk(p) for f in fs)  # noqa: E731
    assert set(names(tmp_path / "with")) - set(names(tmp_path / "plain")) == {DIGEST_JSON, DIGEST_BIN}
    for rel in names(tmp_path / "plain"):  # .zarray and every chunk file, byte for byte
        with open(tmp_path / "plain" / rel, "rb") as a, open(tmp_path / "with" / rel, "rb") as b:
            assert a.read() == b.read(), rel
    assert plain.digest_grid is None
    with pytest.raises(ValueError):
        plain.digest_records()


def test_recreating_removes_a_stale_manifest(tmp_path):
    _write(tmp_path / "a", _volume())
    assert os.path.exists(tmp_path / "a" / DIGEST_JSON) and os.path.exists(tmp_path / "a" / DIGEST_BIN)
    arr = MiniZarrArray.create(str(tmp_path / "a"), SHAPE, CHUNKS, np.uint16)  # overwritten without the option
    assert not os.path.exists(tmp_path / "a" / DIGEST_JSON) and not os.path.exists(tmp_path / "a" / DIGEST_BIN)
    assert arr.digest_grid is None
    arr[0, 0, :4] = 1  # and writing does not bring one back
    assert not os.path.exists(tmp_path / "a" / DIGEST_BIN)
    again = MiniZarrArray.create(str(tmp_path / "a"), SHAPE, CHUNKS, np.uint16, digests=True)  # re-created with it: empty
    assert not again.digest_records()["count"].any()
    # a manifest of another geometry is not this array's
    other = MiniZarrArray.create(str(tmp_path / "b"), (1, 1, 8, 70, 100), CHUNKS, np.uint16, digests=True)
    shutil.copy(tmp_path / "b" / DIGEST_JSON, tmp_path / "a" / DIGEST_JSON)
    assert other.digest_grid == (2, 3, 4) and MiniZarrArray.open(str(tmp_path / "a")).digest_grid is None


def test_what_a_manifest_covers():
    for shape, chunks, dtype in [((1, 2) + ZYX, CHUNKS, np.uint16), (SHAPE, (1, 1, 4, 32, 32), np.float32),
                                 ((70, 100), (32, 32), np.uint16), ((2,) + ZYX, (1, 4, 32, 32), np.uint16)]:  # fmt: skip
        with pytest.raises(ValueError):
            MiniZarrArray.create("/nonexistent/never-created", shape, chunks, dtype, digests=True)
    assert not os.path.exists("/nonexistent")


def test_two_writers_of_disjoint_chunk_rows(tmp_path):
    """Ranks write disjoint ranges of the one file rank 0 created; nothing is merged."""
    vol = _volume(3)
    single = _write(tmp_path / "single", vol)
    MiniZarrArray.create(str(tmp_path / "two"), SHAPE, CHUNKS, np.uint16, digests=True)
    ranks = [MiniZarrArray.open(str(tmp_path / "two")) for _ in range(2)]
    ranks[1][0, 0, 12:22] = vol[12:22]  # chunk rows 3 .. 5, written first
    ranks[0][0, 0, 0:12] = vol[0:12]  # chunk rows 0 .. 2
    with open(tmp_path / "single" / DIGEST_BIN, "rb") as a, open(tmp_path / "two" / DIGEST_BIN, "rb") as b:
        assert a.read() == b.read()
    # and with the records handed over explicitly, as the device path's writers do
    rec = single.digest_records()
    MiniZarrArray.create(str(tmp_path / "three"), SHAPE, CHUNKS, np.uint16, digests=True)
    ranks = [MiniZarrArray.open(str(tmp_path / "three")) for _ in range(2)]
    ranks[1].set_digest_records(4, rec[48:72])
    ranks[0].set_digest_records(0, rec[0:48])
    assert np.array_equal(ranks[0].digest_records(), rec)
    for first, part in [(5, rec[48:72]), (-1, rec[:12]), (0, rec[:7])]:
        with pytest.raises(ValueError):
            ranks[0].set_digest_records(first, part)
    assert np.array_equal(ranks[0].digest_records(), rec)


def test_verify_store_is_clean_on_an_untouched_store(tmp_path):
    arr = _write(tmp_path / "g" / "0", _smooth_volume(), "blosc")
    small = MiniZarrArray.create(str(tmp_path / "g" / "1"), (1, 1, 11, 35, 50), CHUNKS, np.uint16, compressor="blosc", digests=True)
    small[0, 0] = _smooth_volume()[::2, ::2, ::2]
    for path, n_arrays, n_chunks in [(tmp_path / "g" / "0", 1, 72), (tmp_path / "g", 2, 72 + 3 * 2 * 2)]:
        rep = integrity.verify_store(str(path), device=None)
        assert rep["bad"] == [] and rep["arrays"] == n_arrays and rep["chunks"] == n_chunks
    fresh = integrity.digest_store(str(tmp_path / "g" / "0"), device=None, io_threads=3)
    assert np.array_equal(fresh, arr.digest_records())


def _bad(path):
    return [(os.path.basename(p), n, reason) for p, n, reason in integrity.verify_store(str(path), device=None)["bad"]]


def test_verify_store_names_exactly_the_damaged_chunk(tmp_path):
    vol = _smooth_volume()
    # a flipped payload byte in a raw chunk
    raw = _write(tmp_path / "raw", vol, None)
    p = _chunk_file(raw, 17)
    blob = bytearray(open(p, "rb").read())
    blob[1001] ^= 0x10
    open(p, "wb").write(bytes(blob))
    assert _bad(tmp_path / "raw") == [("raw", 17, "digest")]
    # a chunk file replaced by a neighbour's valid file
    shutil.copy(_chunk_file(raw, 30), _chunk_file(raw, 31))
    assert _bad(tmp_path / "raw") == [("raw", 17, "digest"), ("raw", 31, "digest")]
    # a deleted chunk whose voxels were not fill_value: it reads back as fill
    os.remove(_chunk_file(raw, 71))
    assert _bad(tmp_path / "raw") == [("raw", 17, "digest"), ("raw", 31, "digest"), ("raw", 71, "digest")]

    # a truncated Blosc chunk
    bl = _write(tmp_path / "blosc", vol, "blosc")
    p = _chunk_file(bl, 40)
    blob = open(p, "rb").read()
    assert len(blob) < 4 * 32 * 32 * 2  # (really compressed)
    open(p, "wb").write(blob[: len(blob) // 2])
    rep = integrity.verify_store(str(tmp_path / "blosc"), device=None)
    assert [(n, r) for _, n, r in rep["bad"]] == [(40, "undecodable")]
    assert rep["detail"][(str(tmp_path / "blosc"), 40)]  # the host decoder's error
    with pytest.raises(ValueError, match="chunk 40"):
        integrity.digest_store(str(tmp_path / "blosc"), device=None)
    # a flipped byte inside a compressed payload: the decoder refuses it, or it decodes to other voxels
    p = _chunk_file(bl, 5)
    blob = bytearray(open(p, "rb").read())
    blob[len(blob) // 2] ^= 0x40
    open(p, "wb").write(bytes(blob))
    got = _bad(tmp_path / "blosc")
    assert [(n) for _, n, _ in got] == [5, 40] and got[0][2] in ("digest", "undecodable") and got[1][2] == "undecodable"


def test_unrecorded_chunks_and_missing_manifests(tmp_path):
    vol = _volume(5)
    arr = MiniZarrArray.create(str(tmp_path / "g" / "0"), SHAPE, CHUNKS, np.uint16, digests=True)
    arr[0, 0, :20] = vol[:20]  # chunk row 5 is never written
    assert _bad(tmp_path / "g" / "0") == [("0", n, "unrecorded") for n in range(60, 72)]
    plain = MiniZarrArray.create(str(tmp_path / "g" / "1"), SHAPE, CHUNKS, np.uint16)
    plain[0, 0] = vol
    rep = integrity.verify_store(str(tmp_path / "g"), device=None)
    assert rep["arrays"] == 2 and rep["chunks"] == 72
    assert rep["bad"][-1] == (str(tmp_path / "g" / "1"), None, "no manifest") and len(rep["bad"]) == 13
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError):  # neither an array nor a group of numbered arrays
        integrity.verify_store(str(tmp_path / "empty"), device=None)


def test_a_torn_manifest_is_reported_and_the_other_arrays_are_still_checked(tmp_path):
    vol = _volume(6)
    for lvl in ("0", "1", "2"):
        _write(tmp_path / "g" / lvl, vol)
    with open(tmp_path / "g" / "1" / DIGEST_BIN, "r+b") as f:
        f.truncate(100)  # neither whole records nor the grid's number
    os.remove(_chunk_file(MiniZarrArray.open(str(tmp_path / "g" / "2")), 9))
    rep = integrity.verify_store(str(tmp_path / "g"), device=None)
    assert rep["arrays"] == 3 and rep["chunks"] == 144
    assert rep["bad"] == [(str(tmp_path / "g" / "1"), None, "bad manifest"), (str(tmp_path / "g" / "2"), 9, "digest")]
    assert rep["detail"][(str(tmp_path / "g" / "1"), None)]
