"""The Blosc-LZ4 encoder (``csrc/dsx_lz4_enc.h``: a hash-table match finder that writes LZ4 blocks, in the split-stream
container c-blosc 1.21 writes for LZ4 with byte shuffle) built on the host: as ``dsx_blosc_encode_ref_ex`` (mode
``"lz4"``), ``dsx_blosc_encode_lz4`` and ``dsx_io_write_chunks_blosc_lz4`` of the library, and with g++ from
``tests/host/lz4_enc_check.cpp`` (also under ASan / UBSan).  Every frame of tests/lz4_enc_cases.py must decode to its
chunk through the pure-Python reader of that file, liblz4, the real c-blosc, ``dsx_blosc_decode`` and the host build of
the device decoder, keep the rules of the LZ4 block format, and show what its case is named for.  No GPU needed."""

import ctypes
import json
import os
import struct
import subprocess

import lz4_enc_cases as lc
import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

HERE = os.path.dirname(os.path.abspath(__file__))
REAL_BLOSC = "/opt/conda/lib/libblosc.so.1"
LZ4_CONFIG = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


def _liblz4():
    for name in ("liblz4.so.1", "liblz4.so"):
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.LZ4_decompress_safe.restype = ctypes.c_int
        lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        return lib
    return None


def _real_blosc():
    if not os.path.exists(REAL_BLOSC):
        return None
    lib = ctypes.CDLL(REAL_BLOSC)
    lib.blosc_decompress_ctx.restype = ctypes.c_int
    lib.blosc_decompress_ctx.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.blosc_compress_ctx.restype = ctypes.c_int
    lib.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]  # fmt: skip
    return lib


def _build(tmp_path_factory, flags):
    exe = str(tmp_path_factory.mktemp("lz4enc") / "lz4_enc_check")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, os.path.join(HERE, "host", "lz4_enc_check.cpp")],
                   check=True)  # fmt: skip
    return exe


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return _build(tmp_path_factory, ["-O2"])


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return _build(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _encode_gxx(exe, tmp_path, chunks, clevel=5):
    chunks = np.ascontiguousarray(chunks, dtype=np.uint16)
    src, fr, of = (str(tmp_path / x) for x in ("in.raw", "frames.bin", "offsets.bin"))
    chunks.tofile(src)
    subprocess.run([exe, src, str(chunks.nbytes // chunks.shape[0]), str(clevel), fr, of], check=True)
    with open(fr, "rb") as f:
        frames = f.read()
    return frames, np.fromfile(of, np.int64)


@pytest.fixture(scope="module")
def table():
    """The case table with the frames of the library's host build: ``[(name, chunks, frames, offsets)]``."""
    out = []
    for name, chunks in lc.cases() + [("image bricks", lc.image_bricks())]:
        frames, offsets = eng_mod.blosc_encode_ref(chunks, clevel=5, mode="lz4")
        assert len(offsets) == chunks.shape[0] + 1 and offsets[0] == 0 and offsets[-1] == len(frames), name
        out.append((name, chunks, frames, offsets))
    return out


def _frames_of(entry):
    name, chunks, frames, offsets = entry
    for i in range(chunks.shape[0]):
        yield name, i, chunks[i].tobytes(), frames[offsets[i] : offsets[i + 1]]


def test_python_reader_and_the_format_rules(table):
    """(a) the pure-Python container reader and LZ4 block decoder; the walker over every coded stream; frames of at
    most nbytes + 16; the header fields; per case, what it is named for."""
    for entry in table:
        for name, i, raw, frame in _frames_of(entry):
            assert len(frame) <= len(raw) + 16, (name, i)
            assert lc.py_frame_read(frame) == raw, (name, i)
        if entry[0] != "image bricks":
            lc.check_expectations(entry[0], entry[2], entry[3])
    bricks = table[-1]
    seen = lc.check_expectations("noisy low, constant high", bricks[2], bricks[3])  # (stored low planes, coded high planes)
    assert "chained length" in seen and len(bricks[2]) < 0.75 * bricks[1].nbytes


def test_liblz4_decodes_every_coded_stream(table):
    """(b) LZ4_decompress_safe per stream."""
    lib = _liblz4()
    if lib is None:
        pytest.skip("liblz4 is not on this machine")
    coded = 0
    for entry in table:
        for name, i, raw, frame in _frames_of(entry):
            head, streams = lc.frame_streams(frame)
            blocks = {}
            for b, j, n, data in streams:
                if len(data) == n:
                    blocks[b] = blocks.get(b, b"") + data
                    continue
                buf = ctypes.create_string_buffer(n)
                assert lib.LZ4_decompress_safe(data, buf, len(data), n) == n, (name, i, b, j)
                blocks[b] = blocks.get(b, b"") + buf.raw
                coded += 1
            if not head["memcpyed"]:
                got = b"".join(np.frombuffer(blocks[b], np.uint8).reshape(2, -1).T.tobytes() for b in sorted(blocks))
                assert got == raw, (name, i)
    assert coded > 40


def test_real_cblosc_and_the_native_reader_decode_every_frame(table):
    """(c) the real c-blosc, where present; (d) dsx_blosc_decode (its LZ4 streams go through liblz4)."""
    blosc, lz4 = _real_blosc(), _liblz4()
    if blosc is None and lz4 is None:
        pytest.skip("neither c-blosc nor liblz4 is on this machine")
    for entry in table:
        for name, i, raw, frame in _frames_of(entry):
            if blosc is not None and raw:
                back = ctypes.create_string_buffer(len(raw))
                assert blosc.blosc_decompress_ctx(frame, back, len(raw), 1) == len(raw), (name, i)
                assert back.raw == raw, (name, i)
            if lz4 is not None:
                assert mini_zarr.blosc_decode(frame, len(raw)) == raw, (name, i)


def test_every_chunk_goes_to_the_device_decoder_and_decodes(table, tmp_path):
    """(e) the frames as chunk files through dsx_io_read_frames_ex(DSX_ZDEC_ANY) and dsx_blosc_decode_ref."""
    for k, (name, chunks, frames, offsets) in enumerate(table):
        n, nbytes = chunks.shape[0], chunks.nbytes // chunks.shape[0]
        if nbytes == 0:
            continue
        paths = [str(tmp_path / "c{}.{}".format(k, i)) for i in range(n)]
        for i, p in enumerate(paths):
            with open(p, "wb") as f:
                f.write(frames[offsets[i] : offsets[i + 1]])
        packed, tasks, routes = eng_mod.io_read_frames(paths, nbytes, mode=eng_mod.ZDEC_ANY)
        assert np.all(routes[:n] == eng_mod.ROUTE_DEVICE), name
        out, status = eng_mod.blosc_decode_ref(packed, tasks, nbytes * n)
        assert not status.any(), (name, status)
        assert out.tobytes() == chunks.tobytes(), name


def test_gxx_builds_write_the_librarys_bytes(table, check_exe, asan_exe, tmp_path):
    """tests/host/lz4_enc_check.cpp, plain and under ASan / UBSan: the bytes of blosc_encode_ref(mode="lz4")."""
    for name, chunks, frames, offsets in table:
        if chunks.shape[1] == 0:
            continue
        for exe in (check_exe, asan_exe):
            f, o = _encode_gxx(exe, tmp_path, chunks)
            assert np.array_equal(o, offsets) and f == frames, name
    bricks = table[-1][1]
    stored = eng_mod.blosc_encode_ref(bricks, clevel=0, mode="lz4")
    assert _encode_gxx(asan_exe, tmp_path, bricks, clevel=0)[0] == stored[0]
    for i in range(bricks.shape[0]):
        frame = stored[0][stored[1][i] : stored[1][i + 1]]
        assert frame[2] & lc.MEMCPYED and lc.py_frame_read(frame) == bricks[i].tobytes()


def _stream(exe, tmp_path, data):
    src, dst = str(tmp_path / "s.in"), str(tmp_path / "s.out")
    with open(src, "wb") as f:
        f.write(data)
    subprocess.run([exe, "--stream", src, dst], check=True)
    with open(dst, "rb") as f:
        return f.read()


def test_streams_of_12_and_13_bytes_and_other_short_ones(asan_exe, tmp_path):
    """The encoder core on bare streams (a frame of 2-byte elements has no stream of 13 bytes): under 13 bytes literals
    only -- 1 + n bytes, so stored --, and a stream is never coded into its own length or more."""
    rs = np.random.RandomState(5)
    for n in (1, 2, 5, 11, 12, 13, 14, 63, 64, 65, 76, 77, 78, 129, 200):
        for data in (bytes(n), bytes(rs.randint(0, 256, n).astype(np.uint8)), (b"ab" * n)[:n]):
            block = _stream(asan_exe, tmp_path, data)
            if block:
                assert n >= 13 and len(block) < n
                lc.check_stream_rules(block, n)
                assert lc.lz4_block_decode(block, n) == data
            else:  # stored: what the rules allow would not have been shorter
                assert n < 77 or data != bytes(n)  # (zeros: position 64 may open a match from 77 bytes on)
    # a coded stream that ends in a repeat from 12 ... 9 bytes before the end: the repeat stays literals
    for back, length in ((12, 7), (11, 6), (10, 5), (9, 4)):
        data = bytes(lc._late_repeat(rs, back, length))
        seqs = lc.check_stream_rules(_stream(asan_exe, tmp_path, data), len(data))
        assert [s[1:] for s in seqs] == [(1, lc.LATE_ZEROS - 64), (0, 0)] and seqs[-1][0] == len(data) - lc.LATE_ZEROS
    assert _stream(asan_exe, tmp_path, bytes(12)) == b"" and _stream(asan_exe, tmp_path, bytes(13)) == b""
    # zeros: the 64 literals of the first group (token, one chain byte), offset, one chain byte, the last 5 literals
    assert len(_stream(asan_exe, tmp_path, bytes(200))) == 2 + 64 + 2 + 1 + 6


def test_modes_and_refusals():
    assert eng_mod.ZENC_MODES == {"literals": 0, "runs": 1, "lz4": 3}
    bricks = lc.image_bricks(1)
    with pytest.raises(ValueError):
        eng_mod.blosc_encode_ref(bricks, mode="lz")
    lib = eng_mod.load_library()
    buf, off = np.empty(bricks.nbytes + 16, np.uint8), np.zeros(2, np.int64)
    for mode in (2, 4, -1):
        rc = lib.dsx_blosc_encode_ref_ex(bricks.ctypes.data_as(ctypes.c_void_p), 1, bricks.nbytes, 2, 5,
                                         buf.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), mode)
        assert rc != 0, mode
    # the one-frame form and the mode of the batch form write the same frame; clevel 1 ... 9 encode alike, 0 stores
    want = eng_mod.blosc_encode_ref(bricks, clevel=5, mode="lz4")[0]
    for clevel in (1, 5, 9):
        assert mini_zarr.blosc_encode(bricks.tobytes(), 2, clevel=clevel, shuffle=True, cname="lz4") == want
    stored = mini_zarr.blosc_encode(bricks.tobytes(), 2, clevel=0, cname="lz4")
    assert stored[2] & lc.MEMCPYED and len(stored) == bricks.nbytes + 16
    assert mini_zarr.blosc_encode(b"", 2, cname="lz4") == struct.pack("<BBBBIII", 2, 1, 0x23, 2, 0, 0, 16)
    for kw in (dict(typesize=4), dict(typesize=2, shuffle=False), dict(typesize=2, cname="lz4hc")):
        with pytest.raises(NotImplementedError):
            mini_zarr.blosc_encode(bytes(64), **{"cname": "lz4", **kw})


def test_mini_zarr_writes_and_reads_an_lz4_store(tmp_path):
    if _liblz4() is None:
        pytest.skip("liblz4 is not on this machine: the store cannot be read back")
    vol = synth.synthetic_stack(8, 96, 160)
    arr = MiniZarrArray.create(str(tmp_path / "a.zarr"), (1, 1, 8, 96, 160), (1, 1, 8, 64, 64), np.uint16, compressor=LZ4_CONFIG)
    arr[0, 0] = vol
    arr[0, 0, 2:5, 10:20, 30:40] = 7  # (a partial write reads the chunk back)
    vol[2:5, 10:20, 30:40] = 7
    again = MiniZarrArray.open(str(tmp_path / "a.zarr"))
    assert np.array_equal(again[0, 0], vol)
    assert again.blosc_write_params() == (5, 2, True, "lz4")
    with open(again._chunk_path((0, 0, 0, 0, 0)), "rb") as f:
        frame = f.read()
    assert frame == eng_mod.blosc_encode_ref(np.ascontiguousarray(vol[:, :64, :64]).reshape(1, -1), clevel=5, mode="lz4")[0]
    assert lc.py_frame_read(frame) == np.ascontiguousarray(vol[:, :64, :64]).tobytes()
    # shuffle -1 (automatic) at item size 2 is the byte shuffle
    auto = MiniZarrArray.create(str(tmp_path / "b.zarr"), (4, 64), (4, 64), np.int16, compressor={**LZ4_CONFIG, "shuffle": -1})
    auto[...] = np.arange(256, dtype=np.int16).reshape(4, 64)
    assert np.array_equal(auto[...], np.arange(256, dtype=np.int16).reshape(4, 64))


@pytest.mark.parametrize("config, dtype", [
    ({"id": "blosc", "cname": "zlib", "clevel": 5, "shuffle": 1, "blocksize": 0}, np.uint16),
    ({**LZ4_CONFIG, "cname": "lz4hc"}, np.uint16), ({**LZ4_CONFIG, "cname": "blosclz"}, np.uint16),
    ({**LZ4_CONFIG, "cname": "snappy"}, np.uint16), ({**LZ4_CONFIG, "shuffle": 2}, np.uint16),
    ({**LZ4_CONFIG, "shuffle": 0}, np.uint16), ({**LZ4_CONFIG, "blocksize": 65536}, np.uint16),
    (LZ4_CONFIG, np.uint8), (LZ4_CONFIG, np.float32), ({**LZ4_CONFIG, "shuffle": -1}, np.uint8),
])  # fmt: skip
def test_what_stays_read_only(tmp_path, config, dtype):
    arr = MiniZarrArray.create(str(tmp_path / "r.zarr"), (64, 64), (64, 64), dtype, compressor=config)
    with pytest.raises(NotImplementedError, match="read-only"):
        arr[...] = 1
    assert not os.path.exists(arr._chunk_path((0, 0)))


def test_host_writer_writes_the_encoders_frames(tmp_path):
    """dsx_io_write_chunks_blosc_lz4 on the I/O threads: the files are the frames of blosc_encode_ref(mode="lz4")."""
    bricks = np.concatenate([lc.image_bricks(2), np.zeros((1, 64 * 128 * 128), np.uint16)])
    frames, off = eng_mod.blosc_encode_ref(bricks, clevel=5, mode="lz4")
    lib = eng_mod.load_library()
    n = bricks.shape[0]
    paths = [str(tmp_path / "w{}".format(i)) for i in range(n)]
    cp = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    dp = (ctypes.c_void_p * n)(*[bricks[i].ctypes.data for i in range(n)])
    nb = (ctypes.c_size_t * n)(*[bricks[i].nbytes for i in range(n)])
    assert lib.dsx_io_write_chunks_blosc_lz4(None, cp, dp, nb, n, 3, 5) == 0
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            assert f.read() == frames[off[i] : off[i + 1]], i
    nb[0] = 7  # an odd byte count is no array of uint16
    assert lib.dsx_io_write_chunks_blosc_lz4(None, cp, dp, nb, 1, 1, 5) != 0


def size_guard_bricks():
    """The five bricks of the size guard: four (64, 128, 128) bricks of a synthetic stack and the brick of test_blosc."""
    from test_blosc import _brick

    stack = synth.synthetic_stack(64, 256, 256)
    bricks = [np.ascontiguousarray(stack[:, 128 * y : 128 * y + 128, 128 * x : 128 * x + 128]) for y in range(2) for x in range(2)]
    return np.stack([b.reshape(-1) for b in bricks + [_brick()]])


def test_size_stays_within_2_percent_of_the_real_cblosc():
    """Yardstick: the real c-blosc 1.21 at lz4, clevel 5, byte shuffle (blosc_compress_ctx).  Bound 1.02 x its total (a
    Python model of the finder gave 1.005 x).  Measured: 1.0053 x (profiles/device_codec_lz4_sizes.json)."""
    blosc = _real_blosc()
    if blosc is None:
        pytest.skip("the real c-blosc is not on this machine")
    bricks = size_guard_bricks()
    frames, off = eng_mod.blosc_encode_ref(bricks, clevel=5, mode="lz4")
    ours, theirs = [], []
    for i in range(bricks.shape[0]):
        raw = bricks[i].tobytes()
        dest = ctypes.create_string_buffer(len(raw) + 16)
        got = blosc.blosc_compress_ctx(5, 1, 2, len(raw), raw, dest, len(raw) + 16, b"lz4", 0, 1)
        assert 0 < got < len(raw)
        theirs.append(got)
        ours.append(int(off[i + 1] - off[i]))
    ratio = sum(ours) / sum(theirs)
    print("Blosc-LZ4 bytes: this encoder", ours, "c-blosc 1.21 lz4 clevel 5", theirs, "ratio %.4f" % ratio)
    with open(os.path.join(os.path.dirname(HERE), "profiles", "device_codec_lz4_sizes.json")) as f:
        recorded = json.load(f)
    assert recorded["encoder_bytes"] == ours  # (the record is of this encoder)
    assert ratio <= 1.02, (ours, theirs)
