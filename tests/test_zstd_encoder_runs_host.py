"""The runs mode of the device Blosc-zstd encoder (``csrc/dsx_zstd_enc.h`` ``kModeRuns``: runs of >= 8 equal bytes of
a zstd block as offset-1 matches, predefined FSE tables, RLE / raw / Huffman literals), built on the host: with g++ from
``tests/host/zstd_enc_runs_check.cpp`` and as ``dsx_blosc_encode_ref_ex`` of the library.  Every frame must decode to the
chunk's bytes through libzstd, ``dsx_blosc_decode``, the real c-blosc where the image has it, and the host build of the
device decoder (``dsx_io_read_frames`` + ``dsx_blosc_decode_ref``); no frame may be larger than the entropy-only one;
and the synthetic bricks must come within 5 % of the host writer's bytes.  No GPU needed."""

import ctypes
import os
import subprocess

import numpy as np
import pytest
from test_zstd_encoder_host import _bricks, _check_all

import test_zstd_encoder_host as base
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr

HERE = os.path.dirname(os.path.abspath(__file__))
R = 8          # kMinRun of csrc/dsx_zstd_enc.h
SEQ_CAP = 1024  # kSeqCap
ZBLOCK = 128 * 1024


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zencruns") / "zstd_enc_runs_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                    os.path.join(HERE, "host", "zstd_enc_runs_check.cpp")], check=True)  # fmt: skip
    return exe


def _encode_gxx(exe, tmp_path, chunks, clevel=3, mode=1):
    chunks = np.ascontiguousarray(chunks, dtype=np.uint16)
    n = chunks.shape[0]
    src, fr, of = (str(tmp_path / x) for x in ("in.raw", "frames.bin", "offsets.bin"))
    chunks.tofile(src)
    subprocess.run([exe, src, str(chunks.nbytes // n), str(clevel), str(mode), fr, of], check=True)
    with open(fr, "rb") as f:
        frames = f.read()
    return frames, np.fromfile(of, np.int64)


def _encode_both(exe, tmp_path, chunks, clevel=3):
    """g++ build and library build of the runs mode agree byte for byte; mode 0 of the new entry point is the old one."""
    frames, offsets = _encode_gxx(exe, tmp_path, chunks, clevel)
    frames2, offsets2 = eng_mod.blosc_encode_ref(chunks, clevel, mode="runs")
    assert frames == frames2 and np.array_equal(offsets, offsets2)
    old = eng_mod.blosc_encode_ref(chunks, clevel)
    for other in (_encode_gxx(exe, tmp_path, chunks, clevel, mode=0), eng_mod.blosc_encode_ref(chunks, clevel, mode="literals")):
        assert other[0] == old[0] and np.array_equal(other[1], old[1])
    return frames, offsets


def zstd_blocks(zframe):
    """The blocks of a zstd frame of the encoder: ``(type, literals type or None, Number_of_Sequences)`` each; type and
    literals type 0 raw, 1 RLE, 2 compressed."""
    pos = 5 + {0: 1, 1: 2, 2: 4}[zframe[4] >> 6]
    out = []
    while True:
        h = int.from_bytes(zframe[pos : pos + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        assert btype != 3
        if btype == 2:
            b = zframe[pos + 3 : pos + 3 + size]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:
                hdr = {0: 1, 2: 1, 1: 2, 3: 3}[sf]
                regen = (b[0] >> 3) if hdr == 1 else int.from_bytes(b[:hdr], "little") >> 4
                sp = hdr + (regen if lt == 0 else 1)
            else:
                assert sf == 3  # the encoder writes four streams and the 5-byte header
                sp = 5 + ((int.from_bytes(b[:5], "little") >> 22) & 0x3FFFF)
            s0 = b[sp]
            nseq = s0 if s0 < 128 else ((s0 - 128) << 8) + b[sp + 1] if s0 < 255 else b[sp + 1] + (b[sp + 2] << 8) + 0x7F00
            out.append((2, lt, nseq))
        else:
            out.append((btype, None, 0))
        pos += 3 + (1 if btype == 1 else size)
        if last:
            assert pos == len(zframe)
            return out


def frame_blocks(frame):
    """zstd_blocks of every Blosc block of a frame of the encoder that is a zstd frame."""
    import struct

    _, _, flags, _, nbytes, blocksize, _ = struct.unpack("<BBBBIII", frame[:16])
    if flags & 0x2:
        return []
    out = []
    for b in range(-(-nbytes // blocksize)):
        pos = struct.unpack("<i", frame[16 + 4 * b : 20 + 4 * b])[0]
        cs = struct.unpack("<i", frame[pos : pos + 4])[0]
        if cs != min(blocksize, nbytes - b * blocksize):
            out += zstd_blocks(frame[pos + 4 : pos + 4 + cs])
    return out


def check_all(frames, offsets, chunks, tmp_path):
    """_check_all of the entropy-only tests (libzstd, dsx_blosc_decode, c-blosc), then the frames as chunk files
    through dsx_io_read_frames and the host build of the device decoder.  Returns the zstd blocks seen."""
    chunks = np.ascontiguousarray(chunks, dtype=np.uint16)
    n = chunks.shape[0]
    nbytes = chunks.nbytes // n
    saved = base._zstd_block_kinds
    base._zstd_block_kinds = lambda zframe: set()  # (it reads a Huffman tree in every compressed block)
    try:
        _check_all(frames, offsets, chunks)
    finally:
        base._zstd_block_kinds = saved
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / "chunk.{}".format(i)))
        with open(paths[-1], "wb") as f:
            f.write(frames[offsets[i] : offsets[i + 1]])
    packed, tasks, routes = eng_mod.io_read_frames(paths, nbytes)
    assert np.all(routes[:n] == eng_mod.ROUTE_DEVICE)
    out, status = eng_mod.blosc_decode_ref(packed, tasks, nbytes * n)
    assert not status.any(), status
    assert out.tobytes() == chunks.tobytes()
    blocks = []
    for i in range(n):
        blocks += frame_blocks(frames[offsets[i] : offsets[i + 1]])
    return blocks


def planes(low, high):
    """uint16 chunks whose byte-shuffled Blosc block is the bytes ``low`` then the bytes ``high``."""
    return np.asarray(low, np.uint16) | (np.asarray(high, np.uint16) << 8)


def edge_cases():
    """``(name, chunks)``: the edges of the runs mode.  Full chunks have 131 072 elements: the low bytes are zstd block
    0 of the Blosc block (noise unless said otherwise) and the high bytes, where the runs are, zstd block 1.

    Not here, because no input produces it: literals that are all equal.  Neighbouring runs differ, so a block that
    leaves equal literals is one run -- an RLE block -- and an RLE literals section is never chosen."""
    rs = np.random.RandomState(21)
    n = ZBLOCK
    noise = rs.randint(0, 256, n)
    cases = []

    def add(name, high):
        high = np.atleast_2d(high)
        cases.append((name, planes(np.resize(noise, high.shape), high)))

    add("all-equal block", np.full(n, 7))
    rows = []
    for length in (R - 1, R, R + 1):  # 300 runs of one length between single bytes, then bytes without runs
        row = (np.arange(n) % 2) * 3 + rs.randint(0, 2, n) * 8
        row[: 300 * (length + 2)] = np.resize(np.r_[np.full(length, 5), 9, 11], 300 * (length + 2))
        rows.append(row)
    add("runs of R - 1, R, R + 1", np.stack(rows))
    first, last, both = (np.arange(n) % 2 + rs.randint(0, 2, n) * 4 for _ in range(3))
    first[:100] = 3
    last[-100:] = 4
    both[:R] = 7
    both[-R:] = 7
    add("run at the first / the last byte", np.stack([first, last, both]))
    one = np.full(n, 200)
    one[0] = 1
    add("one byte, then 131 071 equal ones", one)
    # periods of a run of 300 and 255 single bytes (256 literals each) behind a prefix of p single bytes: the four
    # literal streams begin at, just before and just after the first byte of a run, and inside the single bytes
    singles = np.arange(255) % 7 + 1
    body = np.resize(np.r_[np.full(300, 77), singles], n)
    rows = [np.r_[np.resize(singles, p), body][:n] for p in (0, 1, 4, 255)]
    add("runs at the literal-stream boundaries", np.stack(rows))
    rows = []
    for keep in (2, 63, 64):  # `keep` long runs of alternating values leave `keep` literals
        rows.append(10 + (np.arange(n) * keep // n) % 2)
    add("2, 63, 64 literals left", np.stack(rows))
    # 14 563 runs of R bytes, one single byte between them; the run values cycle through 200 (a run of a cheap value is
    # not worth a sequence, and the block would stay entropy-only)
    period = np.repeat(np.arange(n // (R + 1) + 1) % 200, R + 1)[:n]
    period[:: R + 1] = 255
    add("period R + 1 over the sequence cap", period)
    m = 131072 + 30000
    cases.append(("partial last Blosc block", planes(rs.randint(0, 256, (2, m)),
                                                      np.repeat(rs.randint(0, 4, (2, m // 100 + 1)), 100, axis=1)[:, :m])))  # fmt: skip
    cases.append(("under 128 bytes", planes(rs.randint(0, 256, (3, 40)), np.full((3, 40), 2))))
    cases.append(("200 bytes", planes(rs.randint(0, 4, (3, 100)), np.full((3, 100), 2))))
    cases.append(("random bytes", rs.randint(0, 65536, (2, 131072)).astype(np.uint16)))
    return cases


def test_length_codes_match_the_decoders_baselines(check_exe):
    subprocess.run([check_exe, "--codes"], check=True)


def test_bricks_have_sequences_decode_everywhere_and_come_close_to_the_host_writer(check_exe, tmp_path):
    """Measured (host build, profiles/device_codec_runs_sizes.json): _bricks(8) 7 059 189 bytes in runs mode against
    7 772 074 entropy-only (0.908 x) and 7 039 648 from the host writer, zstd level 5 (1.003 x)."""
    bricks = _bricks(8)
    frames, offsets = _encode_both(check_exe, tmp_path, bricks)
    blocks = check_all(frames, offsets, bricks, tmp_path)
    assert any(nseq > 0 for _, _, nseq in blocks)
    assert all(nseq <= SEQ_CAP for _, _, nseq in blocks)
    old_frames, old_offsets = eng_mod.blosc_encode_ref(bricks)
    assert np.all(np.diff(offsets) <= np.diff(old_offsets))
    host = sum(len(mini_zarr.blosc_encode(b.tobytes(), 2, clevel=3, shuffle=True)) for b in bricks)
    print("runs", len(frames), "entropy-only", len(old_frames), "host writer", host)
    assert len(frames) <= 1.05 * host, (len(frames), host)
    assert len(frames) <= 0.95 * len(old_frames), (len(frames), len(old_frames))


@pytest.mark.parametrize("case", range(len(edge_cases())))
def test_edges(check_exe, tmp_path, case):
    name, chunks = edge_cases()[case]
    frames, offsets = _encode_both(check_exe, tmp_path, chunks)
    blocks = check_all(frames, offsets, chunks, tmp_path)
    old_frames, old_offsets = eng_mod.blosc_encode_ref(chunks)
    assert np.all(np.diff(offsets) <= np.diff(old_offsets)), name
    seqs = [nseq for _, _, nseq in blocks]
    if name == "all-equal block":
        assert blocks[-1] == (1, None, 0)  # still an RLE block
    elif name == "runs of R - 1, R, R + 1":
        assert [max(s for _, _, s in frame_blocks(frames[offsets[i] : offsets[i + 1]])) for i in range(3)] == [0, 300, 300]
    elif name == "one byte, then 131 071 equal ones":
        assert blocks[-1] == (2, 0, 1)  # two raw literals, one sequence
    elif name == "2, 63, 64 literals left":
        assert [b for b in blocks if b[2]] == [(2, 0, 2), (2, 0, 63), (2, 2, 64)]  # raw, raw, Huffman literals
    elif name == "period R + 1 over the sequence cap":
        assert max(seqs) == SEQ_CAP
    elif name in ("random bytes", "under 128 bytes"):
        assert frames == old_frames and not any(seqs)
    elif name == "runs at the literal-stream boundaries":
        assert [(t, lt, nseq >= 236) for t, lt, nseq in blocks if nseq] == [(2, 2, True)] * 4  # Huffman literals
    elif name == "partial last Blosc block":
        assert sum(1 for s in seqs if s) >= 4  # the full and the partial Blosc block of both chunks


def test_unknown_mode_is_refused():
    with pytest.raises(ValueError):
        eng_mod.blosc_encode_ref(np.zeros((1, 64), np.uint16), mode="lz")
    lib = eng_mod.load_library()
    frames = np.zeros(256, np.uint8)
    offsets = np.zeros(2, np.int64)
    src = np.zeros(64, np.uint16)
    rc = lib.dsx_blosc_encode_ref_ex(src.ctypes.data_as(ctypes.c_void_p), 1, 128, 2, 3,
                                     frames.ctypes.data_as(ctypes.c_void_p), offsets.ctypes.data_as(ctypes.c_void_p), 2)  # fmt: skip
    assert rc == -1 and b"mode" in lib.dsx_last_error(None)
