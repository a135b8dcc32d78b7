"""The zstd decoder of the device path (``csrc/dsx_zstd_dec.h``), built on the host: with g++ from
``tests/host/zstd_dec_check.cpp`` (also under ASan / UBSan) and as ``dsx_blosc_decode_ref`` of the library.  Frames
made by libzstd (through ctypes) must decode to libzstd's bytes exactly; a small frame walker proves that the corpus
exercises every block, literal and sequence mode; Blosc frames go through the native frame reader
(``dsx_io_read_frames``) and the reference decoder; malformed frames end in an error status.  No GPU needed."""

import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import zdec_cases as zc  # (it imports this module in turn: neither uses the other while it loads)
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "blosc_frames.npz")
LEVELS = (-5, -1, 1, 3, 5, 9, 12, 19, 22)
ZSTD_c_compressionLevel, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 100, 200, 201


def _zstd():
    lib = ctypes.CDLL("libzstd.so.1")
    lib.ZSTD_compressBound.restype = ctypes.c_size_t
    lib.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    lib.ZSTD_compress.restype = ctypes.c_size_t
    lib.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.ZSTD_compress2.restype = ctypes.c_size_t
    lib.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.ZSTD_createCCtx.restype = ctypes.c_void_p
    lib.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    lib.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    lib.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.ZSTD_decompress.restype = ctypes.c_size_t
    lib.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return lib


def zstd_compress(data, level, content_size=True, checksum=False):
    lib = _zstd()
    cap = lib.ZSTD_compressBound(len(data))
    buf = ctypes.create_string_buffer(cap)
    if content_size and not checksum:
        n = lib.ZSTD_compress(buf, cap, data, len(data), level)
    else:
        cc = lib.ZSTD_createCCtx()
        lib.ZSTD_CCtx_setParameter(cc, ZSTD_c_compressionLevel, level)
        lib.ZSTD_CCtx_setParameter(cc, ZSTD_c_contentSizeFlag, 1 if content_size else 0)
        lib.ZSTD_CCtx_setParameter(cc, ZSTD_c_checksumFlag, 1 if checksum else 0)
        n = lib.ZSTD_compress2(cc, buf, cap, data, len(data))
        lib.ZSTD_freeCCtx(cc)
    assert not lib.ZSTD_isError(n)
    return buf.raw[:n]


def _token_text(n, seed):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=rng.integers(2, 9)).astype(np.uint8)) for _ in range(300)]
    out, total = [], 0
    while total < n:
        if out and rng.random() < 0.1:  # a long repeat of what came before
            k = int(rng.integers(1, min(len(out), 40) + 1))
            piece = b" ".join(out[-k:])
        else:
            piece = words[int(rng.zipf(1.3)) % len(words)]
        out.append(piece)
        total += len(piece) + 1
    return b" ".join(out)[:n]


def _shuffle2(raw):
    a = np.frombuffer(raw[: len(raw) // 2 * 2], np.uint8).reshape(-1, 2)
    return a[:, 0].tobytes() + a[:, 1].tobytes() + raw[len(raw) // 2 * 2 :]


def corpus_data():
    """name -> bytes: image bricks (byte-shuffled and not), token text, zeros, random bytes, odd sizes."""
    plane = synth.synthetic_plane(3, 512, 1024).astype(np.uint16).tobytes()  # 1 MiB
    rng = np.random.default_rng(7)
    d = {
        "brick_shuffled": _shuffle2(plane),
        "brick": plane,
        "text": _token_text(300_000, 1),
        "zeros": bytes(200_000),
        "random": rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(),
        "empty": b"",
        "one": b"x",
        "seven": b"abcabca",
        "small_text": _token_text(5000, 3),  # 2-byte content size
    }
    sparse = np.zeros(300_000, np.uint8)
    sparse[rng.integers(0, sparse.size, 3000)] = 1  # Treeless literals, Repeat offset / match-length tables
    d["sparse"] = sparse.tobytes()
    for n in (128 * 1024 - 1, 128 * 1024, 128 * 1024 + 1):
        d["brick_{}".format(n)] = _shuffle2(plane)[:n]
    d["mib"] = _shuffle2(plane)[: 1 << 20]
    return d


def corpus_frames():
    """(name, frame, data): every corpus buffer at every level, plus frames without a content size."""
    out = []
    for name, data in corpus_data().items():
        for lv in LEVELS:
            out.append(("{}@{}".format(name, lv), zstd_compress(data, lv), data))
        out.append(("{}@3/nosize".format(name), zstd_compress(data, 3, content_size=False), data))
    return out


@pytest.fixture(scope="module")
def corpus():
    return corpus_frames()


def zstd_decode_ref(frame, n):
    """One bare zstd frame through dsx_blosc_decode_ref (a single zstd task without un-shuffle): (status, bytes)."""
    task = eng_mod.decode_task(0, 0, len(frame), n, eng_mod.TASK_ZSTD)
    out, status = eng_mod.blosc_decode_ref(np.frombuffer(frame, np.uint8), task, n)
    return int(status[0]), (out.tobytes() if status[0] == 0 else None)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return zc.build_check_exe(str(tmp_path_factory.mktemp("zdec") / "zstd_dec_check"))


def _decode_gxx(exe, tmp_path, items):
    rec, out = str(tmp_path / "rec.bin"), str(tmp_path / "out.bin")
    zc.write_records(rec, items)
    subprocess.run([exe, "decode", rec, out], check=True)
    blob = open(out, "rb").read()
    res, at = [], 0
    for _, want in items:
        st = struct.unpack("<i", blob[at : at + 4])[0]
        at += 4
        data = None
        if st == 0:
            data = blob[at : at + want]
            at += want
        res.append((st, data))
    return res


def test_corpus_matches_libzstd_gxx(check_exe, tmp_path, corpus):
    res = _decode_gxx(check_exe, tmp_path, [(f, len(d)) for _, f, d in corpus])
    for (name, _, data), (st, got) in zip(corpus, res):
        assert st == 0, (name, st)
        assert got == data, name


def test_corpus_matches_libzstd_ref(corpus):
    for name, frame, data in corpus:
        st, got = zstd_decode_ref(frame, len(data))
        assert st == 0, (name, st)
        assert got == data, name


# ---- coverage: a walker of the frames counts the cases they use ---------------------------------------------------
def _walk(frame):
    """Set of the cases one frame uses (block types, literal types x streams, weight forms, sequence modes)."""
    cases = set()
    d = frame[4]
    single, fcs_flag = (d >> 5) & 1, d >> 6
    p = 5 + (0 if single else 1)
    p += {0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fcs_flag]
    cases.add("fcs{}".format({0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fcs_flag]))
    cases.add("single" if single else "window")
    while True:
        bh = int.from_bytes(frame[p : p + 3], "little")
        last, btype, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        cases.add(("block", btype))
        if btype == 2:
            b = frame[p : p + bs]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:
                hdr = {0: 1, 2: 1, 1: 2, 3: 3}[sf]
                regen = b[0] >> 3 if hdr == 1 else (b[0] >> 4) + (b[1] << 4) + ((b[2] << 12) if hdr == 3 else 0)
                size = regen if lt == 0 else 1
                cases.add(("lit", lt))
            else:
                hdr = {0: 3, 1: 3, 2: 4, 3: 5}[sf]
                v = int.from_bytes(b[:hdr], "little")
                size = {3: (v >> 14) & 0x3FF, 4: (v >> 18) & 0x3FFF, 5: (v >> 22) & 0x3FFFF}[hdr]
                cases.add(("lit", lt, 1 if sf == 0 else 4))
                if lt == 2:
                    cases.add(("weights", "fse" if b[hdr] < 128 else "direct"))
            s = b[hdr + size :]
            if s[0] != 0:
                q = 1 if s[0] < 128 else (2 if s[0] < 255 else 3)
                modes = s[q]
                for k, nm in enumerate(("LL", "OF", "ML")):
                    cases.add(("seq", nm, (modes >> (6 - 2 * k)) & 3))
            else:
                cases.add(("seq", "none"))
            p += bs
        else:
            p += bs if btype == 0 else 1
        if last:
            return cases


def _hand_frame():
    """A frame whose one compressed block uses RLE literals and the RLE mode for all three sequence tables (libzstd
    writes neither on the corpus): literals "bb", then one sequence (literal length 2, offset code 2 with extra bits
    0b00 -> offset value 4 -> offset 1, match length code 7 -> 10) -> "b" * 12."""
    lit = bytes([1 | (2 << 3)]) + b"b"
    seq = bytes([1, 0b01010100, 2, 2, 7]) + bytes([0b100])  # count, modes, LL / OF / ML symbols, bits + end mark
    block = lit + seq
    out = b"b" * 12
    hdr = struct.pack("<I", 0xFD2FB528) + bytes([0x20, len(out)])
    bh = 1 | (2 << 1) | (len(block) << 3)
    return hdr + bh.to_bytes(3, "little") + block, out


def _hand_frame_fcs8():
    """Frame_Content_Size in 8 bytes (single segment), one Raw block."""
    out = b"0123456789ab"
    hdr = struct.pack("<I", 0xFD2FB528) + bytes([0xE0]) + struct.pack("<Q", len(out))
    return hdr + (1 | (len(out) << 3)).to_bytes(3, "little") + out, out


def test_corpus_covers_every_mode(corpus):
    """Every case occurs in some frame, and each frame that brings a new case decodes (dsx_blosc_decode_ref) to its
    data: the cases are not only present but decoded."""
    seen = set()
    for name, frame, data in corpus + [("hand", *_hand_frame()), ("hand fcs8", *_hand_frame_fcs8())]:
        cases = _walk(frame)
        if cases - seen:
            assert zstd_decode_ref(frame, len(data)) == (0, data), name
        seen |= cases
    need = {("block", 0), ("block", 1), ("block", 2), ("lit", 0), ("lit", 1), ("lit", 2, 1), ("lit", 2, 4),
            ("lit", 3, 1), ("lit", 3, 4), ("weights", "fse"), ("weights", "direct"), "single", "window",
            "fcs0", "fcs1", "fcs2", "fcs4", "fcs8", ("seq", "none")}  # fmt: skip
    need |= {("seq", nm, m) for nm in ("LL", "OF", "ML") for m in range(4)}
    assert need <= seen, sorted(map(str, need - seen))


def test_hand_assembled_frames(check_exe, tmp_path):
    for frame, out in (_hand_frame(), _hand_frame_fcs8()):
        assert _zstd_decompress(frame, len(out)) == out  # libzstd agrees on the hand-made frame
        assert _decode_gxx(check_exe, tmp_path, [(frame, len(out))])[0] == (0, out)
        assert zstd_decode_ref(frame, len(out)) == (0, out)


def _zstd_decompress(frame, n):
    lib = _zstd()
    buf = ctypes.create_string_buffer(max(n, 1))
    got = lib.ZSTD_decompress(buf, n, frame, len(frame))
    assert not lib.ZSTD_isError(got)
    return buf.raw[:got]


# ---- Blosc level: the native frame reader + the reference decoder ----------------------------------------------------
def blosc_frame_cblosc_layout(raw, blocksize, zlevel, shuffle=True):
    """A c-blosc 1.x frame as c-blosc lays it out for zstd: version 2, typesize 2, byte shuffle, "don't split",
    blocks of `blocksize` (32 KiB at clevel 1, 128 KiB at 3, 1 MiB at 9), one zstd frame per block (or the block
    stored when zstd does not make it smaller)."""
    n = len(raw)
    nblocks = -(-n // blocksize)
    table, body = [], b""
    at = 16 + 4 * nblocks
    for b in range(nblocks):
        blk = raw[b * blocksize : (b + 1) * blocksize]
        if shuffle:
            blk = _shuffle2(blk)
        z = zstd_compress(blk, zlevel)
        part = blk if len(z) >= len(blk) else z
        table.append(at + len(body))
        body += struct.pack("<I", len(part)) + part
    flags = (0x1 if shuffle else 0) | 0x10 | (4 << 5)
    hdr = struct.pack("<BBBBIII", 2, 1, flags, 2, n, blocksize, 16 + 4 * nblocks + len(body))
    return hdr + b"".join(struct.pack("<I", t) for t in table) + body


def _zlib_inside(raw):
    """A c-blosc 1.x frame with zlib inside (byte shuffle, one unsplit block): the host route."""
    import zlib

    comp = zlib.compress(_shuffle2(raw), 1)
    body = struct.pack("<I", 20) + struct.pack("<I", len(comp)) + comp
    return struct.pack("<BBBBIII", 2, 1, 0x1 | 0x10 | (3 << 5), 2, len(raw), len(raw), 16 + len(body)) + body


def blosc_frames_corpus():
    """[(chunk_bytes, frames, raws)]: groups of chunk files of one size.  None = a missing file."""
    bricks = [synth.synthetic_plane(k, 256, 2048).tobytes() for k in range(3)]  # 1 MiB each
    cb = len(bricks[0])
    groups = []
    for shuffle in (True, False):
        frames = [mini_zarr.blosc_encode(bricks[lv % 3], 2, lv, shuffle) for lv in range(1, 10)]
        groups.append((cb, frames + [None], [bricks[lv % 3] for lv in range(1, 10)] + [None]))
    arr = np.stack([np.frombuffer(b, np.uint16) for b in bricks])
    fr, off = eng_mod.blosc_encode_ref(arr)
    groups.append((cb, [fr[off[i] : off[i + 1]] for i in range(3)], bricks))
    zeros = bytes(cb)
    groups.append((cb, [mini_zarr.blosc_encode(zeros, 2, 5), mini_zarr.blosc_encode(zeros, 2, 0)], [zeros, zeros]))
    return groups


def golden_frames():
    """(frame, raw) of every committed c-blosc 1.21.0 frame (tests/golden/blosc_frames.npz)."""
    from test_blosc import payload

    g = np.load(GOLDEN)
    out, n = [], 0
    while "frame_%03d" % n in g.files:
        _, _, _, _, kind, seed, nbytes, _ = str(g["case_%03d" % n]).split()
        out.append((g["frame_%03d" % n].tobytes(), payload(kind, int(seed), int(nbytes))))
        n += 1
    return out


# the frames the routing table (csrc/dsx_io.h blosc_device_route, README) sends to the host decoder
HOST_ROUTE_KINDS = ("other inner codec", "bit shuffle", "typesize != 2", "split streams", "zstd checksum",
                    "blocks under 8 KiB")


def _route_cases():
    """(name, frame, raw, route) of frames named by the routing table."""
    raw = synth.synthetic_plane(9, 128, 1024).tobytes()  # 256 KiB
    dev = blosc_frame_cblosc_layout(raw, 128 * 1024, 3)
    cases = [
        ("device zstd", dev, raw, 0),
        ("device no shuffle", blosc_frame_cblosc_layout(raw, 32 * 1024, 1, False), raw, 0),
        ("memcpyed", mini_zarr.blosc_encode(raw, 2, 0), raw, 0),
        # a chunk takes at most chunk_bytes / 8192 + 1 tasks: 8 KiB blocks still go to the device, 4 KiB blocks do not
        ("device 8 KiB blocks", blosc_frame_cblosc_layout(raw, 8192, 3), raw, 0),
        ("blocks under 8 KiB", blosc_frame_cblosc_layout(raw, 4096, 3), raw, 1),
        ("other inner codec", _zlib_inside(raw), raw, 1),
    ]
    # the same zstd blocks with the checksum flag: the host decodes them
    blk = _shuffle2(raw)
    z = zstd_compress(blk, 3, checksum=True)
    body = struct.pack("<I", len(z)) + z
    ck = struct.pack("<BBBBIII", 2, 1, 0x1 | 0x10 | (4 << 5), 2, len(raw), len(raw), 20 + len(body))
    cases.append(("zstd checksum", ck + struct.pack("<I", 20) + body, raw, 1))
    # split streams, bit shuffle, another type size: flags changed on a device frame -> host route (the host reader
    # then rejects the frame or decodes other bytes -- the route alone is checked here)
    split = bytearray(dev)
    split[2] &= ~0x10
    cases.append(("split streams", bytes(split), None, 1))
    bit = bytearray(dev)
    bit[2] |= 0x4
    cases.append(("bit shuffle", bytes(bit), None, 1))
    ts = bytearray(dev)
    ts[3] = 4
    cases.append(("typesize != 2", bytes(ts), None, 1))
    return cases


def test_frames_route_as_the_table_says(tmp_path):
    cases = _route_cases()
    assert {name for name, _, _, route in cases if route == 1} == set(HOST_ROUTE_KINDS)
    for name, frame, raw, route in cases:
        p = str(tmp_path / name.replace(" ", "_"))
        with open(p, "wb") as f:
            f.write(frame)
        if raw is None:  # what the host reader makes of these frames does not matter: only that it is the host
            try:
                _, _, routes = eng_mod.io_read_frames([p], 256 * 1024)
            except eng_mod.DsxError as e:  # only the host route decodes while reading: its error names the file
                assert os.path.basename(p) in str(e), name
            else:
                assert int(routes[0]) == eng_mod.ROUTE_HOST, name
            continue
        packed, tasks, routes = eng_mod.io_read_frames([p], len(raw))
        assert int(routes[0]) == route, name
        out, st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any(), name
        assert out.tobytes() == raw, name


def test_blosc_corpus_through_reader_and_ref(tmp_path):
    for gi, (cb, frames, raws) in enumerate(blosc_frames_corpus()):
        paths = []
        for i, f in enumerate(frames):
            p = str(tmp_path / "g{}_{}".format(gi, i))
            if f is not None:
                with open(p, "wb") as fh:
                    fh.write(f)
            paths.append(p)
        packed, tasks, routes = eng_mod.io_read_frames(paths, cb, fill_value=0xBEEF)
        out, st = eng_mod.blosc_decode_ref(packed, tasks, cb * len(frames))
        assert not st.any()
        for i, (f, r) in enumerate(zip(frames, raws)):
            got = out[i * cb : (i + 1) * cb].tobytes()
            if f is None:
                assert routes[i] == eng_mod.ROUTE_FILL and got == struct.pack("<H", 0xBEEF) * (cb // 2)
            else:
                assert routes[i] == eng_mod.ROUTE_DEVICE, (gi, i)
                assert got == r == mini_zarr.blosc_decode(f, cb), (gi, i)
    for k, (frame, raw) in enumerate(golden_frames()):
        p = str(tmp_path / "golden{}".format(k))
        with open(p, "wb") as fh:
            fh.write(frame)
        packed, tasks, _ = eng_mod.io_read_frames([p], len(raw))
        out, st = eng_mod.blosc_decode_ref(packed, tasks, len(raw))
        assert not st.any() and out.tobytes() == raw, k


# ---- malformed input: CPU sanitizers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return zc.build_check_exe(str(tmp_path_factory.mktemp("zdec_asan") / "zstd_dec_check"), sanitize=True)


def test_mutations_under_sanitizers(asan_exe, tmp_path, corpus):
    pick = [c for c in corpus if c[0] in ("text@3", "sparse@9", "brick_131073@5", "seven@1", "small_text@19")]
    assert len(pick) == 5
    pick.append(("hand",) + _hand_frame())
    rec = str(tmp_path / "rec.bin")
    zc.write_records(rec, [(f, len(d)) for _, f, d in pick])
    r = subprocess.run([asan_exe, "mutate", rec, "600", "1"], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))  # fmt: skip
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    seen = {}
    for line in r.stdout.strip().splitlines():
        st, cnt = map(int, line.split())
        seen[st] = cnt
    assert sum(v for k, v in seen.items() if k != 0) > 1000  # most mutations are caught


def _frame_with_block(block, out_len, last=True, btype=2):
    hdr = struct.pack("<I", 0xFD2FB528) + bytes([0xA0]) + struct.pack("<I", out_len)
    return hdr + ((1 if last else 0) | (btype << 1) | (len(block) << 3)).to_bytes(3, "little") + block


def _broken_frames():
    """name -> (frame, output bytes, expected status of dsx_zstd_dec.h)."""
    good, out = _hand_frame()
    n = len(out)
    cases = {}
    reserved = bytearray(good)
    reserved[4] |= 0x08
    cases["reserved bit"] = (bytes(reserved), n, 4)
    big = struct.pack("<I", 0xFD2FB528) + bytes([0xA0]) + struct.pack("<I", 200000)
    big += (1 | (1 << 1) | ((128 * 1024 + 1) << 3)).to_bytes(3, "little") + b"x"
    cases["block over 128 KiB"] = (big, 200000, 5)
    # sequences with an FSE table of accuracy log 10 for literal lengths (limit 9)
    acc = bytes([1 | (2 << 3)]) + b"b" + bytes([1, 0b10000000, 5])  # RLE literals, 1 sequence, LL FSE; log = 5 + 5
    cases["accuracy log too large"] = (_frame_with_block(acc + b"\x00" * 8, n), n, 8)
    # Huffman weights in direct form whose sum needs more than 11 bits (a weight of 12)
    hw = bytes([2 | (0 << 2) | ((8 & 0xF) << 4), (8 >> 4) | ((5 & 0x3) << 6), 5 >> 2])  # 1 stream, regen 8, size 5
    hw += bytes([127 + 2, 0xC1]) + b"\x01\x01\x01"
    cases["Huffman weights over the limit"] = (_frame_with_block(hw + b"\x00", 8), 8, 7)
    # offset before the start of the output: literals "bb", then offset code 3 with extra bits 0b000 -> offset value 8
    # -> offset 5, with 2 bytes written
    seq = bytes([1, 0b01010100, 2, 3, 7]) + bytes([0b1000])
    cases["offset before the start"] = (_frame_with_block(bytes([1 | (2 << 3)]) + b"b" + seq, n), n, 11)
    # literals longer than the block: a Raw literals header claiming 31 bytes in a 5-byte block
    cases["literals longer than the block"] = (_frame_with_block(bytes([31 << 3]) + b"abcd", n), n, 1)
    # sequence bitstream overrun: offset code 20 needs 20 extra bits, the stream has 2
    seq = bytes([1, 0b01010100, 2, 20, 7]) + bytes([0b100])
    cases["sequence bitstream overrun"] = (_frame_with_block(bytes([1 | (2 << 3)]) + b"b" + seq, n), n, 10)
    cases["output short"] = (good, n + 1, 12)
    cases["output long"] = (good, n - 1, 12)
    return cases


def test_broken_frames_return_their_status(check_exe, tmp_path):
    cases = _broken_frames()
    names = list(cases)
    res = _decode_gxx(check_exe, tmp_path, [(cases[k][0], cases[k][1]) for k in names])
    for k, (st, _) in zip(names, res):
        assert st == cases[k][2], (k, st)
        assert zstd_decode_ref(cases[k][0], cases[k][1])[0] == cases[k][2], k
