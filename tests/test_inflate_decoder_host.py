"""The zlib and blosclz decoders of the device path (``csrc/dsx_inflate.h``), built on the host: as
``dsx_blosc_decode_ref`` of the library and with g++ from ``tests/host/zdec_task_check.cpp`` (also under ASan /
UBSan, a program of its own).  ``dsx_io_read_frames_ex`` in mode ``DSX_ZDEC_ALL`` routes frames with zlib or blosclz
inside to the device and modes 0 and 1 keep them on the host; the frames of the real c-blosc 1.21.0 decode to their
payload; every valid zlib stream is one Python's ``zlib`` decodes to the same bytes; hand-assembled streams cover
what its encoder does not write; malformed streams end in a status.  No GPU needed."""

import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import blosc_any_frames as baf
import inflate_cases as ic
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr
from aind_smartspim_destripe_amd import zarr_destriper as zd

E = eng_mod


def _read(tmp_path, frame, nbytes, mode, name="chunk"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(frame)
    return E.io_read_frames([p], nbytes, mode=mode)


def _on_the_device_route(tmp_path, name, frame, raw):
    packed, tasks, routes = _read(tmp_path, frame, len(raw), E.ZDEC_ALL)
    assert int(routes[0]) == E.ROUTE_DEVICE, name
    assert packed.nbytes == len(frame), name  # the frame travels as it is
    out, st = E.blosc_decode_ref(packed, tasks, len(raw))
    assert not st.any(), (name, st)
    assert out.tobytes() == raw, name
    assert mini_zarr.blosc_decode(frame, len(raw)) == raw, name  # the pinned host reader agrees on what the frame holds
    return tasks


def _host_in_modes_0_and_1(tmp_path, name, frame, raw):
    for mode in (E.ZDEC_ZSTD, E.ZDEC_ANY):
        packed, tasks, routes = _read(tmp_path, frame, len(raw), mode)
        assert int(routes[0]) == E.ROUTE_HOST and len(tasks) == 1 and int(tasks["kind"][0]) == E.TASK_COPY, (name, mode)
        out, st = E.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any() and out.tobytes() == raw, (name, mode)


# ---- the streams ---------------------------------------------------------------------------------------------------------
def test_the_blosclz_encoder_of_the_tests_round_trips():
    rng = np.random.default_rng(1)
    for data in (baf.shuffle2(baf.brick(1, 40000)), bytes(5000), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
                 b"abcabcabcabcabcabcabcabcabcabcabcabcabc", b"short", b"a", b""):  # fmt: skip
        z = ic.blosclz_compress(data)
        assert ic.blosclz_decompress_py(z, len(data)) == data
        if len(data) >= 16:  # ... and the pinned host decoder (blosclz_decompress of csrc/dsx_io.h) reads it
            frame = baf.blosc_frame(data, len(data), baf.BLOSCLZ, baf.NOSHUFFLE, split=False, streams={(0, 0): z})
            assert mini_zarr.blosc_decode(frame, len(data)) == data
    assert len(ic.blosclz_compress(bytes(5000))) < 40
    chunk = baf.shuffle2(baf.brick(2, 131072))
    z = ic.blosclz_compress_runs(chunk)
    assert ic.blosclz_decompress_py(z, len(chunk)) == chunk and len(z) < len(chunk)


def test_zlib_streams_decode_to_their_input():
    """Levels 0, 1, 6, 9 x the four strategies x the inputs of the issue, periods 1 .. 300, full flushes, several
    blocks; then the hand-assembled streams.  One table, canaries between the outputs."""
    streams = ic.zlib_corpus() + ic.hand_streams()
    names = " | ".join(n for n, _, _ in streams)
    for need in ("empty level 0 default", "one level 9 fixed", "noise level 6 huffman", "runs level 1 rle", "period 1 |",
                 "period 300", "full flushes", "several blocks", "repeat code over both alphabets",
                 "single-code distance set", "dynamic block without a match", "stored blocks of LEN 0",
                 "distances 32768 and 32767", "lengths 258 and 257"):  # fmt: skip
        assert need in names + " |", need
    for flag in zc.FLAGS:
        t = ic.zlib_table(streams, flag)
        out, st = zc.run_ref(t)
        zc.check(t, out, st, "zlib corpus, flag {:#x}".format(flag))


def test_blosclz_corner_cases():
    t = zc.Table()
    for i, (name, z, data) in enumerate(ic.blosclz_hand_streams()):
        t.add(name, z, len(data), E.TASK_BLOSCLZ, data, dst_res=i % 16, src_res=i % 4)
    assert len(t.rows) >= 6
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "blosclz corners")


def test_malformed_zlib_streams_end_in_a_status():
    """Each malformed stream is one ``zlib.decompress`` refuses (or decodes to another length); its neighbours in the
    table decode, and no byte outside a task's destination changes."""
    cases = ic.malformed_streams()
    names = " | ".join(n for n, _, _, _ in cases)
    for need in ("cut at byte", "BTYPE 3", "LEN / NLEN mismatch", "over-subscribed literal/length set",
                 "incomplete literal/length set", "incomplete distance set", "no end-of-block code", "length symbol 286",
                 "distance symbol 30", "distance before the start", "one byte too many", "one byte too few",
                 "wrong Adler-32", "FDICT set", "repeat code with no previous length"):  # fmt: skip
        assert need in names, need
    for name, z, n, _ in cases:
        assert ic.zlib_rejects(z, n), name
    t = ic.malformed_table()
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "malformed zlib")
    for i, name in enumerate(t.names):
        assert (int(st[i]) == 0) == name.startswith("good "), (name, int(st[i]))


def test_malformed_blosclz_streams_end_in_a_status():
    t = zc.Table()
    good = ic.blosclz_hand_streams()[0]
    for i, (name, z, n, st) in enumerate(ic.blosclz_malformed()):
        t.add("good", good[1], len(good[2]), E.TASK_BLOSCLZ, good[2], dst_res=(2 * i) % 16, src_res=(2 * i) % 4)
        t.add(name, z, n, E.TASK_BLOSCLZ, None, status=st, dst_res=(2 * i + 1) % 16, src_res=(2 * i + 1) % 4)
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "malformed blosclz")
    for i, name in enumerate(t.names):
        assert (int(st[i]) == 0) == (name == "good"), (name, int(st[i]))
        if name != "good":  # the pinned host decoder refuses what the shared one refuses
            z = bytes(t.packed[t.rows[i][0] : t.rows[i][0] + t.rows[i][2]])
            n = t.rows[i][3]
            frame = struct.pack("<BBBBIII", 2, 1, 0x10, 2, n, n, 24 + len(z)) + struct.pack("<II", 20, len(z)) + z
            with pytest.raises(Exception):
                mini_zarr.blosc_decode(frame, n)


def test_layout_sweep():
    """Table B for the new kinds: kind x shuffle flag x split form, lengths 0 .. 70 001, every residue of the
    destination mod 16 and of the source mod 4."""
    t, facts = ic.layout_table()
    for kind in (E.TASK_ZLIB, E.TASK_BLOSCLZ):
        for flag in zc.FLAGS:
            for split in (False, True):
                assert any(f["kind"] == kind and f["flag"] == flag and f["split"] == split for f in facts)
    assert {f["dst"] % 16 for f in facts} == set(range(16)) and {f["src"] % 4 for f in facts} == set(range(4))
    assert {f["n"] for f in facts} == set(zc.LENGTHS)
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "B (zlib, blosclz)")


# ---- frames --------------------------------------------------------------------------------------------------------------
def test_routes_device_in_mode_all_host_in_modes_0_and_1(tmp_path):
    raw = baf.brick(7, 65536)
    for codec, kind in ((ic.ZLIB, E.TASK_ZLIB), (baf.BLOSCLZ, E.TASK_BLOSCLZ)):
        for shuffle, flag in ((baf.NOSHUFFLE, 0), (baf.SHUFFLE, E.TASK_SHUFFLE), (baf.BITSHUFFLE, E.TASK_BITSHUFFLE)):
            for split in (True, False):
                name = "codec {} shuffle {} split {}".format(codec, shuffle, split)
                frame = ic.blosc_frame(raw, 32768, codec, shuffle, split)
                tasks = _on_the_device_route(tmp_path, name, frame, raw)
                want = kind | flag | (E.TASK_SPLIT if split else 0)
                assert len(tasks) == 2 and set(int(k) for k in tasks["kind"]) == {want}, (name, tasks["kind"])
                _host_in_modes_0_and_1(tmp_path, name, frame, raw)
    # what mode 1 sends to the device is the same task in mode 3
    for codec in (baf.LZ4, baf.ZSTD):
        dev = baf.blosc_frame(raw, 32768, codec, baf.SHUFFLE, split=True)
        a = _read(tmp_path, dev, len(raw), E.ZDEC_ANY)
        b = _read(tmp_path, dev, len(raw), E.ZDEC_ALL)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2][0] == b[2][0] == 0
    # still the host's in mode 3: another type size, blocks under 8 KiB
    ts4 = bytearray(ic.blosc_frame(raw, 32768, ic.ZLIB, baf.NOSHUFFLE, False))
    ts4[3] = 4
    for name, frame in (("typesize 4", bytes(ts4)), ("4 KiB blocks", ic.blosc_frame(raw, 4096, ic.ZLIB, baf.SHUFFLE, True))):
        packed, tasks, routes = _read(tmp_path, frame, len(raw), E.ZDEC_ALL)
        assert int(routes[0]) == E.ROUTE_HOST, name
        out, st = E.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any() and out.tobytes() == raw, name
    for bad in (2, 4, -1):  # (2 stays refused: tests/test_lz4_decoder_host.py)
        with pytest.raises(E.DsxError):
            E.io_read_frames([str(tmp_path / "chunk")], len(raw), mode=bad)


def test_real_cblosc_frames_of_both_files(tmp_path):
    """tests/golden/blosc_all_frames.npz (blosclz and zlib inside, nine levels, three shuffles) and the blosclz / zlib
    frames of typesize 2 of tests/golden/blosc_frames.npz.  c-blosc 1.21 splits every full block of 2-byte elements,
    whatever the codec; a short last block is one stream: both forms occur."""
    frames = ic.golden_all_frames()
    assert len(frames) == 58
    old = [(c, f, r) for c, f, r in baf.golden_any_frames()[1]
           if c.split()[0] in ("blosclz", "zlib") and int(c.split()[3]) == 2 and len(r) >= 16]  # fmt: skip
    assert len(old) >= 6
    kinds, seen = {}, set()
    for case, frame, raw in frames + old:
        f = case.split()
        memcpyed = bool(frame[2] & 0x2)
        tasks = _on_the_device_route(tmp_path, case, frame, raw)
        if not memcpyed:
            _host_in_modes_0_and_1(tmp_path, case, frame, raw)
            seen.add((f[0], int(f[1]), int(f[2])))
        for k in tasks["kind"]:
            kinds[int(k)] = kinds.get(int(k), 0) + 1
    for kind in (E.TASK_ZLIB, E.TASK_BLOSCLZ):
        for flag in zc.FLAGS:
            assert kinds.get(kind | flag | E.TASK_SPLIT, 0) > 0, (kind, flag, "split")
        assert sum(n for k, n in kinds.items() if k & 0xFF == kind and not k & E.TASK_SPLIT) > 0, (kind, "unsplit")
    for cname in ("blosclz", "zlib"):  # every level and every shuffle mode was coded (not stored whole) at least once
        assert {lv for c, lv, _ in seen if c == cname} == set(range(1, 10)), cname
        assert {sh for c, _, sh in seen if c == cname} == {0, 1, 2}, cname


def test_plain_zlib_chunk_files(tmp_path):
    """``dsx_io_read_zlib_chunks``: one task of kind 5 per chunk file, a fill task for a missing one, and a file that
    does not fit its share of the packed buffer inflated by the reader."""
    rng = np.random.default_rng(3)
    n = 65536
    chunks = [baf.brick(21, n), None, rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n)]
    paths = []
    for i, c in enumerate(chunks):
        paths.append(str(tmp_path / "c{}".format(i)))
        if c is not None:
            with open(paths[-1], "wb") as f:
                f.write(zlib.compress(c, 1))
    assert os.path.getsize(paths[2]) > n + 16
    packed, tasks, routes = E.io_read_frames(paths, n, fill_value=0x1234, zlib_chunks=True)
    assert list(routes) == [E.ROUTE_DEVICE, E.ROUTE_FILL, E.ROUTE_HOST, E.ROUTE_DEVICE]
    by_chunk = {int(t["chunk"]): t for t in tasks}
    assert [int(by_chunk[i]["kind"]) for i in range(4)] == [E.TASK_ZLIB, E.TASK_FILL, E.TASK_COPY, E.TASK_ZLIB]
    assert all(int(t["dst_len"]) == n and int(t["dst"]) == n * int(t["chunk"]) for t in tasks)
    out, st = E.blosc_decode_ref(packed, tasks, 4 * n)
    assert not st.any()
    want = [c if c is not None else struct.pack("<H", 0x1234) * (n // 2) for c in chunks]
    assert out.tobytes() == b"".join(want)
    with open(paths[0], "r+b") as f:  # a stream the reader itself inflates names its file when it is bad
        f.seek(40)
        f.write(b"\xff\xff\xff\xff")
    with open(paths[2], "r+b") as f:
        f.seek(n // 2)
        f.write(b"\x00\x00\x00\x00")
    with pytest.raises(E.DsxError, match="zlib: bad chunk .*c2"):
        E.io_read_frames(paths, n, zlib_chunks=True)


# ---- the g++ build, and malformed input under the sanitizers --------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return zc.build_task_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return zc.build_task_exe(tmp_path_factory, sanitize=True)


def _table_records(t):
    return [(bytes(t.packed[r[0] : r[0] + r[2]]), r[3], r[4]) for r in t.rows]


def _decode(exe, tmp_path, recs):
    rec, out = str(tmp_path / "rec.bin"), str(tmp_path / "out.bin")
    zc.write_records(rec, recs)
    r = subprocess.run([exe, "decode", rec, out], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))  # fmt: skip
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    blob, at, res = open(out, "rb").read(), 0, []
    for _, n, _ in recs:
        st = struct.unpack("<i", blob[at : at + 4])[0]
        at += 4
        res.append((st, blob[at : at + n] if st == 0 else None))
        at += n if st == 0 else 0
    assert at == len(blob)
    return res


@pytest.mark.parametrize("which", ["plain", "sanitizers"])
def test_gxx_build_runs_the_tables(which, check_exe, asan_exe, tmp_path):
    """The corpus, the hand-assembled streams, table B and the malformed streams through the stand-alone program: the
    statuses and bytes of ``dsx_blosc_decode_ref``, and under ASan / UBSan no report.  The program keeps every input
    and output in a buffer of exactly its size."""
    exe = check_exe if which == "plain" else asan_exe
    tables = [ic.zlib_table(ic.zlib_corpus() + ic.hand_streams()), ic.layout_table()[0], ic.malformed_table()]
    bl = zc.Table()
    for name, z, data in ic.blosclz_hand_streams():
        bl.add(name, z, len(data), E.TASK_BLOSCLZ, data)
    for name, z, n, st in ic.blosclz_malformed():
        bl.add(name, z, n, E.TASK_BLOSCLZ, None, status=st)
    tables.append(bl)
    for t in tables:
        _, ref_st = zc.run_ref(t)
        res = _decode(exe, tmp_path, _table_records(t))
        for i, (st, data) in enumerate(res):
            assert st == int(ref_st[i]), (t.names[i], st, int(ref_st[i]))
            if t.expect[i] is not None:
                assert st == 0 and data == t.expect[i], t.names[i]


def test_mutations_under_sanitizers(asan_exe, tmp_path):
    """Every truncation and 300 single-byte mutations of small tasks of every new kind: a status, or status 0 with
    some output -- never a sanitizer report.  A zlib stream carries a checksum: a mutation that changes its bytes is
    detected; overall at least half of the mutations must be."""
    raw = baf.brick(9, 2048)
    recs = []
    for codec, kind in ((ic.ZLIB, E.TASK_ZLIB), (baf.BLOSCLZ, E.TASK_BLOSCLZ)):
        for flag in zc.FLAGS:
            st = zc.stored_form(raw, flag)
            recs.append((ic.code(kind, st), len(raw), kind | flag))
            parts = [ic.code(kind, h) for h in (st[:1024], st[1024:])]
            recs.append((b"".join(struct.pack("<I", len(z)) + z for z in parts), len(raw), kind | flag | E.TASK_SPLIT))
    recs += [(z, len(d), E.TASK_ZLIB) for n, z, d in ic.hand_streams() if len(z) < 200]
    recs.append((ic.deflate(raw, 6, zlib.Z_FIXED), len(raw), E.TASK_ZLIB))
    recs.append((ic.deflate(raw, 0), len(raw), E.TASK_ZLIB))
    rec = str(tmp_path / "rec.bin")
    zc.write_records(rec, recs)
    r = subprocess.run([asan_exe, "mutate", rec, "300", "1"], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))  # fmt: skip
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    total = detected = 0
    for line in r.stdout.strip().splitlines():
        st, same, cnt = map(int, line.split())
        total += cnt
        if st != 0 or not same:
            detected += cnt
    n_cuts = sum(len(d) for d, _, _ in recs)
    assert total == n_cuts + 300 * len(recs)
    print("mutations and truncations: {} of {} detected".format(detected, total))
    assert detected - n_cuts >= 0.5 * (total - n_cuts), (detected, total, n_cuts)


# ---- the public option ---------------------------------------------------------------------------------------------------
def test_device_decode_argument():
    assert zd.device_decode_mode("full") == "full" and zd.device_decode_mode("any") == "any"
    assert zd.device_decode_mode(True) == "zstd" and zd.device_decode_mode(False) is None
    for bad in ("nope", "", "FULL", "all", "zstd", "zlib"):  # ("all" stays refused: tests/test_pyramid_bricks_host.py)
        with pytest.raises(ValueError, match="one of \"any\", \"full\""):
            zd.device_decode_mode(bad)
    assert (E.ZDEC_ALL, E.TASK_ZLIB, E.TASK_BLOSCLZ) == (3, 5, 6)


def test_a_zlib_store_needs_all(tmp_path):
    """A plain-zlib uint16 store: refused with ``True`` and ``"any"`` as before (before anything is written)."""
    from aind_smartspim_destripe_amd import synth
    from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

    p = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(p, (1, 1, 64, 128, 128), (1, 1, 64, 128, 128), np.uint16, compressor="zlib")
    src[0, 0] = np.zeros((64, 128, 128), np.uint16)
    assert zd.device_decode_input_ok(src, "full") and not zd.device_decode_input_ok(src, "any")
    for mode in (True, "any"):
        out = str(tmp_path / "o_{}.zarr".format(mode))
        with pytest.raises(ValueError, match="device_decode needs a Blosc uint16 input"):
            zd.destripe_zarr_store(p, out, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                   prediction_chunksize=(64, 128, 128), output_chunks=(1, 1, 64, 128, 128),
                                   device_decode=mode)  # fmt: skip
