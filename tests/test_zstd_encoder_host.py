"""The Blosc-zstd encoder of the device path (``csrc/dsx_zstd_enc.h``: entropy-only zstd -- RLE / raw / Huffman
literal blocks, no sequences -- in the host writer's Blosc container), built on the host: with g++ from
``tests/host/zstd_enc_check.cpp`` and as ``dsx_blosc_encode_ref`` of the library.  Every frame must decode to the
chunk's bytes through libzstd (the inner zstd frames, read with the independent Python container reader of
``tests/test_blosc.py``), through the repository's ``dsx_blosc_decode``, and through the real c-blosc where the image
has it.  No GPU needed."""

import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr, synth

HERE = os.path.dirname(os.path.abspath(__file__))
REAL_BLOSC = "/opt/conda/lib/libblosc.so.1"
MEMCPYED = 0x2


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zenc") / "zstd_enc_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "host", "zstd_enc_check.cpp")],
                   check=True)  # fmt: skip
    return exe


def _encode_gxx(exe, tmp_path, chunks, clevel=3):
    chunks = np.ascontiguousarray(chunks, dtype=np.uint16)
    n = chunks.shape[0]
    src, fr, of = (str(tmp_path / x) for x in ("in.raw", "frames.bin", "offsets.bin"))
    chunks.tofile(src)
    subprocess.run([exe, src, str(chunks.nbytes // n), str(clevel), fr, of], check=True)
    with open(fr, "rb") as f:
        frames = f.read()
    return frames, np.fromfile(of, np.int64)


def _zstd():
    lib = ctypes.CDLL("libzstd.so.1")
    lib.ZSTD_decompress.restype = ctypes.c_size_t
    lib.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
    lib.ZSTD_getErrorName.restype = ctypes.c_char_p
    lib.ZSTD_getErrorName.argtypes = [ctypes.c_size_t]
    return lib


def _read_with_libzstd(frame):
    """The c-blosc 1.x container read in Python (unsplit blocks, byte shuffle of 2-byte elements); every stream that
    is not stored goes through libzstd's ZSTD_decompress.  Returns (bytes, block kinds seen)."""
    lib = _zstd()
    version, _, flags, typesize, nbytes, blocksize, cbytes = struct.unpack("<BBBBIII", frame[:16])
    assert version == 2 and typesize == 2 and cbytes == len(frame)
    assert flags & 0x1 and flags & 0x10 and flags >> 5 == 4  # shuffle, don't split, zstd
    if flags & MEMCPYED:
        assert len(frame) == 16 + nbytes
        return frame[16:], {"memcpyed"}
    kinds = set()
    out = b""
    for b in range(-(-nbytes // blocksize)):
        bsize = min(blocksize, nbytes - b * blocksize)
        pos = struct.unpack("<i", frame[16 + 4 * b : 20 + 4 * b])[0]
        cs = struct.unpack("<i", frame[pos : pos + 4])[0]
        part = frame[pos + 4 : pos + 4 + cs]
        if cs == bsize:
            blk = part
            kinds.add("stored")
        else:
            assert part[:4] == b"\x28\xb5\x2f\xfd"
            buf = ctypes.create_string_buffer(bsize)
            got = lib.ZSTD_decompress(buf, bsize, part, len(part))
            assert not lib.ZSTD_isError(got), lib.ZSTD_getErrorName(got)
            assert got == bsize
            blk = buf.raw
            kinds |= _zstd_block_kinds(part)
        ne = bsize // 2
        out += np.frombuffer(blk, np.uint8).reshape(2, ne).T.tobytes()
    return out, kinds


def _zstd_block_kinds(zframe):
    fhd = zframe[4]
    pos = 5 + {0: 1, 1: 2, 2: 4}[fhd >> 6]
    kinds = set()
    while True:
        h = int.from_bytes(zframe[pos : pos + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        if btype == 2:
            tree = zframe[pos + 8]
            kinds.add("huffman-fse" if tree < 128 else "huffman-direct")
        kinds.add({0: "raw", 1: "rle", 2: "compressed"}[btype])
        pos += 3 + (1 if btype == 1 else size)
        if last:
            return kinds


def _real_blosc():
    if not os.path.exists(REAL_BLOSC):
        return None
    lib = ctypes.CDLL(REAL_BLOSC)
    lib.blosc_decompress_ctx.restype = ctypes.c_int
    lib.blosc_decompress_ctx.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return lib


def _check_all(frames, offsets, chunks):
    """Every frame decodes to its chunk with libzstd, dsx_blosc_decode and (where present) c-blosc."""
    chunks = np.ascontiguousarray(chunks, dtype=np.uint16)
    n = chunks.shape[0]
    nbytes = chunks.nbytes // n
    assert len(offsets) == n + 1 and offsets[0] == 0 and offsets[-1] == len(frames)
    blosc = _real_blosc()
    kinds = set()
    for i in range(n):
        frame = frames[offsets[i] : offsets[i + 1]]
        raw = chunks[i].tobytes()
        assert len(frame) <= nbytes + 16
        if nbytes == 0:
            assert mini_zarr.blosc_decode(frame, 0) == b""
            continue
        got, k = _read_with_libzstd(frame)
        kinds |= k
        assert got == raw, i
        assert mini_zarr.blosc_decode(frame, nbytes) == raw, i
        if blosc is not None:
            back = ctypes.create_string_buffer(nbytes)
            assert blosc.blosc_decompress_ctx(frame, back, nbytes, 1) == nbytes, i
            assert back.raw == raw, i
    return kinds


def _encode_both(exe, tmp_path, chunks, clevel=3):
    """g++ build and library build of the encoder must agree byte for byte."""
    frames, offsets = _encode_gxx(exe, tmp_path, chunks, clevel)
    frames2, offsets2 = eng_mod.blosc_encode_ref(chunks, clevel)
    assert frames == frames2 and np.array_equal(offsets, offsets2)
    return frames, offsets


def _bricks(n, shape=(64, 128, 128), seed=0):
    out = np.empty((n,) + shape, np.uint16)
    for k in range(n):
        plane = synth.synthetic_plane(seed + k, shape[0] * 4, shape[1] * shape[2] // 4)
        out[k] = plane.reshape(shape)
    return out


def test_synthetic_bricks_decode_everywhere_and_stay_near_the_host_writer(check_exe, tmp_path):
    bricks = _bricks(8)
    frames, offsets = _encode_both(check_exe, tmp_path, bricks)
    kinds = _check_all(frames, offsets, bricks)
    assert "compressed" in kinds and "huffman-fse" in kinds  # the low byte plane uses ~all 256 symbols
    host = sum(len(mini_zarr.blosc_encode(b.tobytes(), 2, clevel=3, shuffle=True)) for b in bricks)
    assert len(frames) <= 1.25 * host, (len(frames), host)
    assert len(frames) < 0.6 * bricks.nbytes


def test_rle_stored_and_short_chunks(check_exe, tmp_path):
    rs = np.random.RandomState(3)
    zero = np.zeros((2, 64, 64, 64), np.uint16)
    zero[1] = 1234  # constant: both byte planes are RLE blocks
    frames, offsets = _encode_both(check_exe, tmp_path, zero)
    assert _check_all(frames, offsets, zero) == {"rle"}
    assert offsets[1] < 80  # header, table, 2 x (length, frame header, 2 RLE blocks)
    noise = rs.randint(0, 65536, (3, 100000), dtype=np.int64).astype(np.uint16)
    frames, offsets = _encode_both(check_exe, tmp_path, noise)
    assert _check_all(frames, offsets, noise) == {"memcpyed"}
    for n in (1, 10, 63):  # chunks under 128 bytes are stored whole
        short = rs.randint(0, 3, (4, n)).astype(np.uint16)
        frames, offsets = _encode_both(check_exe, tmp_path, short)
        assert _check_all(frames, offsets, short) == {"memcpyed"}
    # clevel 0 stores
    frames, offsets = _encode_both(check_exe, tmp_path, _bricks(1, (8, 64, 64)), clevel=0)
    assert _check_all(frames, offsets, _bricks(1, (8, 64, 64))) == {"memcpyed"}


def test_partial_blocks_and_raw_fallback(check_exe, tmp_path):
    rs = np.random.RandomState(5)
    # 2.5 Blosc blocks: the last one is 64 KiB (one zstd block holding both byte planes), and sizes whose zstd
    # blocks end off every boundary
    for n_el in (5 * 65536, 3 * 65536 + 1000, 65536 + 37, 200, 64):
        a = (rs.poisson(40, (2, n_el)) + (rs.rand(2, n_el) < 0.01) * 3000).astype(np.uint16)
        frames, offsets = _encode_both(check_exe, tmp_path, a)
        _check_all(frames, offsets, a)
    # low bytes uniform noise (stored raw zstd block), high bytes constant (RLE) in one frame
    a = rs.randint(0, 256, (2, 131072)).astype(np.uint16) + 0x4100
    frames, offsets = _encode_both(check_exe, tmp_path, a)
    assert {"raw", "rle"} <= _check_all(frames, offsets, a)


@pytest.mark.parametrize("distinct", [1, 2, 128, 129, 256])
def test_literal_alphabets(check_exe, tmp_path, distinct):
    """Low byte planes with 1, 2, 128, 129 and 256 distinct symbols (skewed, so Huffman pays where it can)."""
    rs = np.random.RandomState(distinct)
    p = 1.0 / (np.arange(distinct) + 1.0)
    low = rs.choice(distinct, size=(2, 131072), p=p / p.sum()).astype(np.uint16)  # low / high plane: one zstd block each
    low[:, :distinct] = np.arange(distinct)  # every symbol present
    a = low | np.uint16(7 << 8)
    frames, offsets = _encode_both(check_exe, tmp_path, a)
    kinds = _check_all(frames, offsets, a)
    if distinct == 1:
        assert kinds == {"rle"}
    else:
        assert "compressed" in kinds
    if distinct == 2:
        assert "huffman-direct" in kinds or "huffman-fse" in kinds


def test_fibonacci_histogram_forces_the_length_limit(check_exe, tmp_path):
    """Counts in Fibonacci proportion give an unlimited Huffman code 20+ bits deep: the 11-bit limit must hold and
    the code stay complete."""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    sym = np.repeat(np.arange(24), fib)[: 131072]
    rs = np.random.RandomState(9)
    low = np.resize(rs.permutation(sym), 131072).astype(np.uint16)
    a = np.stack([low, low[::-1]]) | np.uint16(3 << 8)
    frames, offsets = _encode_both(check_exe, tmp_path, a)
    assert "compressed" in _check_all(frames, offsets, a)


def test_ref_rejects_other_types():
    with pytest.raises(ValueError):
        eng_mod.blosc_encode_ref(np.zeros((2, 10), np.float32))
    lib = eng_mod.load_library()
    frames = np.zeros(64, np.uint8)
    offsets = np.zeros(2, np.int64)
    src = np.zeros(16, np.uint8)
    rc = lib.dsx_blosc_encode_ref(src.ctypes.data_as(ctypes.c_void_p), 1, 16, 4, 3,
                                  frames.ctypes.data_as(ctypes.c_void_p), offsets.ctypes.data_as(ctypes.c_void_p))  # fmt: skip
    assert rc == -1 and b"typesize 2" in lib.dsx_last_error(None)
