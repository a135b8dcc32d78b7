"""The device decoder beyond unsplit zstd (``csrc/dsx_lz4_dec.h``: LZ4 blocks; ``csrc/dsx_zdec_task.h``: split streams,
bit un-shuffle), built on
the host: as ``dsx_blosc_decode_ref`` of the library and with g++ from ``tests/host/zdec_task_check.cpp`` (also under
ASan / UBSan).  ``dsx_io_read_frames_ex`` in mode ``DSX_ZDEC_ANY`` routes these frames to the device and mode 0 keeps
them on the host; the frames of the real c-blosc 1.21.0 (``tests/golden/blosc_frames.npz``) decode to their payload;
hand-assembled blocks cover the corners of the formats; malformed tasks end in a status.  No GPU needed."""

import os
import struct
import subprocess

import numpy as np
import pytest

import blosc_any_frames as baf
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr
from aind_smartspim_destripe_amd import zarr_destriper as zd


def _read(tmp_path, frame, nbytes, mode, name="chunk"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(frame)
    return eng_mod.io_read_frames([p], nbytes, mode=mode)


def _decodes_on_the_device_route(tmp_path, name, frame, raw):
    packed, tasks, routes = _read(tmp_path, frame, len(raw), eng_mod.ZDEC_ANY)
    assert int(routes[0]) == eng_mod.ROUTE_DEVICE, name
    assert packed.nbytes == len(frame), name  # the frame travels as it is
    out, st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
    assert not st.any(), (name, st)
    assert out.tobytes() == raw, name
    if baf.have_liblz4():  # the pinned host reader agrees on what the frame holds
        assert mini_zarr.blosc_decode(frame, len(raw)) == raw, name
    return tasks


def test_the_lz4_encoder_of_the_tests_round_trips():
    rng = np.random.default_rng(1)
    for data in (baf.shuffle2(baf.brick(1, 40000)), bytes(5000), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
                 b"abcabcabcabcabcabcabcabcabcabcabcabcabc", b"short"):  # fmt: skip
        z = baf.lz4_compress(data)
        assert baf.lz4_decompress_py(z, len(data)) == data
    assert len(baf.lz4_compress(bytes(5000))) < 40


def test_routes_device_in_mode_any_host_in_mode_zstd(tmp_path):
    """Every frame kind DSX_ZDEC_ANY adds goes to the device in mode 1 and decodes to what was encoded; mode 0 (and
    dsx_io_read_frames itself) keeps it on the host."""
    lib = eng_mod.load_library()
    assert hasattr(lib, "dsx_io_read_frames_ex")
    raw = baf.brick(7, 65536)
    kinds = {
        "lz4 split shuffle": (baf.LZ4, baf.SHUFFLE, True, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT | eng_mod.TASK_SHUFFLE),
        "lz4 unsplit shuffle": (baf.LZ4, baf.SHUFFLE, False, eng_mod.TASK_LZ4 | eng_mod.TASK_SHUFFLE),
        "lz4 split": (baf.LZ4, baf.NOSHUFFLE, True, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT),
        "lz4 split bitshuffle": (baf.LZ4, baf.BITSHUFFLE, True, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT | eng_mod.TASK_BITSHUFFLE),
        "lz4 unsplit bitshuffle": (baf.LZ4, baf.BITSHUFFLE, False, eng_mod.TASK_LZ4 | eng_mod.TASK_BITSHUFFLE),
        "zstd split shuffle": (baf.ZSTD, baf.SHUFFLE, True, eng_mod.TASK_ZSTD | eng_mod.TASK_SPLIT | eng_mod.TASK_SHUFFLE),
        "zstd split": (baf.ZSTD, baf.NOSHUFFLE, True, eng_mod.TASK_ZSTD | eng_mod.TASK_SPLIT),
        "zstd unsplit bitshuffle": (baf.ZSTD, baf.BITSHUFFLE, False, eng_mod.TASK_ZSTD | eng_mod.TASK_BITSHUFFLE),
        "zstd split bitshuffle": (baf.ZSTD, baf.BITSHUFFLE, True, eng_mod.TASK_ZSTD | eng_mod.TASK_SPLIT | eng_mod.TASK_BITSHUFFLE),
    }  # fmt: skip
    for name, (codec, shuffle, split, kind) in kinds.items():
        frame = baf.blosc_frame(raw, 32768, codec, shuffle, split)
        tasks = _decodes_on_the_device_route(tmp_path, name, frame, raw)
        assert len(tasks) == 2 and set(int(k) for k in tasks["kind"]) == {kind}, (name, tasks["kind"])  # one per block
        _, t0, routes = _read(tmp_path, frame, len(raw), eng_mod.ZDEC_ZSTD)
        assert int(routes[0]) == eng_mod.ROUTE_HOST and int(t0["kind"][0]) == eng_mod.TASK_COPY, name
        _, _, routes = eng_mod.io_read_frames([str(tmp_path / "chunk")], len(raw))
        assert int(routes[0]) == eng_mod.ROUTE_HOST, name
    # what mode 0 sends to the device is the same task in mode 1
    dev = baf.blosc_frame(raw, 32768, baf.ZSTD, baf.SHUFFLE, split=False)
    a = _read(tmp_path, dev, len(raw), eng_mod.ZDEC_ZSTD)
    b = _read(tmp_path, dev, len(raw), eng_mod.ZDEC_ANY)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2][0] == b[2][0] == 0
    # still the host's in mode 1: another inner codec, another type size, blocks under 8 KiB
    host = {"blosclz": baf.blosclz_frame(raw[:8192]), "4 KiB blocks": baf.blosc_frame(raw, 4096, baf.LZ4, baf.SHUFFLE, True)}
    ts4 = bytearray(baf.blosc_frame(raw, 32768, baf.LZ4, baf.NOSHUFFLE, False))
    ts4[3] = 4
    host["typesize 4"] = bytes(ts4)
    for name, frame in host.items():
        n = 8192 if name == "blosclz" else len(raw)
        if name == "4 KiB blocks" and not baf.have_liblz4():
            continue  # (the host route decodes while it reads, and needs the library for that)
        if name == "typesize 4" and not baf.have_liblz4():
            continue
        packed, tasks, routes = _read(tmp_path, frame, n, eng_mod.ZDEC_ANY)
        assert int(routes[0]) == eng_mod.ROUTE_HOST, name
        out, st = eng_mod.blosc_decode_ref(packed, tasks, n)
        assert not st.any() and out.tobytes() == raw[:n], name
    with pytest.raises(eng_mod.DsxError):
        eng_mod.io_read_frames([str(tmp_path / "chunk")], len(raw), mode=2)


def test_real_cblosc_frames(tmp_path):
    picked, others = baf.golden_any_frames()
    assert len(picked) >= 12
    assert len(picked) == 17
    kinds = set()
    for case, frame, raw in picked:
        tasks = _decodes_on_the_device_route(tmp_path, case, frame, raw)
        kinds |= set(int(k) for k in tasks["kind"])
    # the real library's frames hold split LZ4 blocks with byte and with bit shuffle, and stored leftover blocks
    assert eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT | eng_mod.TASK_SHUFFLE in kinds
    assert eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT | eng_mod.TASK_BITSHUFFLE in kinds
    n_host = 0
    for case, frame, raw in others:
        cname, _, _, typesize = case.split()[:4]
        memcpyed = bool(frame[2] & 0x2)
        if memcpyed or (cname == "zstd" and int(typesize) == 2):
            continue  # (a copy task, or the zstd frames the device takes)
        if cname in ("lz4", "lz4hc") and not baf.have_liblz4():
            continue
        packed, tasks, routes = _read(tmp_path, frame, len(raw), eng_mod.ZDEC_ANY)
        assert int(routes[0]) == eng_mod.ROUTE_HOST, case
        out, st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any() and out.tobytes() == raw, case
        n_host += 1
    assert n_host >= 20


def test_corner_cases(tmp_path):
    frames = baf.hand_frames()
    names = " | ".join(n for n, _, _ in frames)
    for need in ("offsets 1 2 3", "offset 65535", "one literal run", "stored + coded", "hand-made run stream",
                 "leftover block", "zstd split"):  # fmt: skip
        assert need in names, need
    for name, frame, raw in frames:
        _decodes_on_the_device_route(tmp_path, name, frame, raw)


# ---- the g++ build, and malformed input under the sanitizers --------------------------------------------------------
def _records(tmp_path, frames):
    """One record per task of the frames (mode 1): (task bytes, output bytes, kind), and the bytes it decodes to."""
    recs, want = [], []
    for name, frame, raw in frames:
        packed, tasks, _ = _read(tmp_path, frame, len(raw), eng_mod.ZDEC_ANY)
        out, st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any() and out.tobytes() == raw, name
        for t in tasks:
            s, n = int(t["src"]), int(t["src_len"])
            recs.append((packed[s : s + n].tobytes(), int(t["dst_len"]), int(t["kind"])))
            want.append(raw[int(t["dst"]) : int(t["dst"]) + int(t["dst_len"])])
    return recs, want


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return zc.build_task_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return zc.build_task_exe(tmp_path_factory, sanitize=True)


def test_gxx_build_decodes_the_corpus(check_exe, tmp_path):
    recs, want = _records(tmp_path, baf.hand_frames())
    rec, out = str(tmp_path / "rec.bin"), str(tmp_path / "out.bin")
    zc.write_records(rec, recs)
    subprocess.run([check_exe, "decode", rec, out], check=True)
    blob, at = open(out, "rb").read(), 0
    for (_, n, kind), w in zip(recs, want):
        st = struct.unpack("<i", blob[at : at + 4])[0]
        assert st == 0, (hex(kind), st)
        assert blob[at + 4 : at + 4 + n] == w, hex(kind)
        at += 4 + n
    assert at == len(blob)


def _small_frames():
    """Small frames of every new kind for the mutation run: LZ4 and zstd, split and not, the three shuffles, and the
    hand-made block with the extension bytes."""
    raw = baf.brick(9, 2048)  # (one block: a chunk this small has one task)
    out = [(n, f, r) for n, f, r in baf.hand_frames() if "extension bytes" in n]
    assert len(out) == 1
    for codec in (baf.LZ4, baf.ZSTD):
        for shuffle in (baf.NOSHUFFLE, baf.SHUFFLE, baf.BITSHUFFLE):
            for split in (True, False):
                out.append(("small {} {} {}".format(codec, shuffle, split), baf.blosc_frame(raw, len(raw), codec, shuffle, split), raw))
    return out


def test_mutations_under_sanitizers(asan_exe, tmp_path):
    """Every truncation and 300 single-byte mutations of every task: a status, or status 0 with some output -- never
    a sanitizer report.  At least half of the mutations must be detected (a status, or other bytes than the
    original's): a decoder that checks nothing cannot pass."""
    recs, _ = _records(tmp_path, _small_frames())
    assert len(recs) == 13
    kinds = {k for _, _, k in recs}
    assert {eng_mod.TASK_LZ4, eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT, eng_mod.TASK_ZSTD | eng_mod.TASK_SPLIT,
            eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT | eng_mod.TASK_BITSHUFFLE} <= kinds  # fmt: skip
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
    assert detected - n_cuts >= 0.5 * (total - n_cuts), (detected, total, n_cuts)  # (every truncation is detected)


def test_broken_tasks_return_their_status():
    """The malformed inputs the issue names, each with the status it must give (dsx_zstd_dec.h Status)."""
    good = baf.Lz4Asm().lit(b"abcdefgh").match(3, 20).lit(b"12345").end()
    stream, raw = good
    n = len(raw)

    def status(data, want, kind=eng_mod.TASK_LZ4):
        task = eng_mod.decode_task(0, 0, len(data), want, kind)
        _, st = eng_mod.blosc_decode_ref(np.frombuffer(data, np.uint8), task, want)
        return int(st[0])

    assert status(stream, n) == 0
    for cut in range(len(stream)):
        assert status(stream[:cut], n) != 0, cut
    assert status(stream[:4], n) == 1  # truncated inside the literals
    assert status(stream, n + 1) == 12 and status(stream, n - 1) == 12  # output short / long
    before = baf.lz4_sequence(b"abcdefgh", 9, 20) + baf.lz4_sequence(b"12345")
    assert status(before, n) == 11  # an offset before the start of the output
    zero = bytearray(before)
    zero[9:11] = b"\x00\x00"
    assert status(bytes(zero), n) == 11
    assert status(baf.lz4_sequence(b"abcdefgh", 3, 200) + baf.lz4_sequence(b"12345"), n) == 12  # a match past the output
    assert status(baf.lz4_sequence(b"abcdefgh" * 8), n) == 12  # literals past the output
    assert status(bytes([0xF0]) + b"\xff" * 40, n) == 12  # a literal length that never ends
    assert status(stream + b"\x00", n) != 0
    # split streams: a stream length past the task's bytes, and bytes left over behind the second stream
    two = struct.pack("<I", len(stream)) + stream + struct.pack("<I", len(stream)) + stream
    k = eng_mod.TASK_LZ4 | eng_mod.TASK_SPLIT
    assert status(two, 2 * n, k) == 0
    long = bytearray(two)
    long[0:4] = struct.pack("<I", len(two))
    assert status(bytes(long), 2 * n, k) == 1
    assert status(two + b"\x00", 2 * n, k) == 1
    assert status(two[:-1], 2 * n, k) == 1
    assert status(two, 2 * n + 1, k) == 12


# ---- the public option --------------------------------------------------------------------------------------------------
def test_device_decode_argument():
    assert zd.device_decode_mode(False) is None and zd.device_decode_mode(None) is None
    assert zd.device_decode_mode(True) == "zstd" and zd.device_decode_mode(1) == "zstd"
    assert zd.device_decode_mode("any") == "any"
    for bad in ("nope", "", "ANY", "zstd"):
        with pytest.raises(ValueError):
            zd.device_decode_mode(bad)


def test_device_decode_string_is_checked_before_anything_is_written(tmp_path):
    from aind_smartspim_destripe_amd import synth
    from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

    p = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(p, (1, 1, 64, 128, 128), (1, 1, 64, 128, 128), np.uint16, compressor="blosc")
    src[0, 0] = np.zeros((64, 128, 128), np.uint16)
    out = str(tmp_path / "o.zarr")
    with pytest.raises(ValueError, match="device_decode"):
        zd.destripe_zarr_store(p, out, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                               prediction_chunksize=(64, 128, 128), output_chunks=(1, 1, 64, 128, 128),
                               device_decode="nope")  # fmt: skip
    assert not os.path.exists(out)
