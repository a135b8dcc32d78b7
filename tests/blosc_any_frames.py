"""Test infrastructure for the frames ``DSX_ZDEC_ANY`` sends to the device (``csrc/dsx_lz4_dec.h``): a small greedy LZ4
block encoder, an assembler for hand-made LZ4 blocks, c-blosc's bit shuffle, and the c-blosc 1.x container around
them (LZ4 or zstd inside, split or unsplit blocks, no / byte / bit shuffle).  The frames are trusted because the host
build of the decoder returns the bytes that went in (tests/test_lz4_decoder_host.py) and, where ``liblz4.so.1`` can be
opened, the pinned host reader does too."""

import ctypes
import struct

import numpy as np

from aind_smartspim_destripe_amd import synth

LZ4, ZSTD, BLOSCLZ = 1, 4, 0  # c-blosc's inner codec numbers
NOSHUFFLE, SHUFFLE, BITSHUFFLE = 0, 1, 2


def have_liblz4():
    for name in ("liblz4.so.1", "liblz4.so"):
        try:
            ctypes.CDLL(name)
            return True
        except OSError:
            pass
    return False


# ---- LZ4 blocks ------------------------------------------------------------------------------------------------------
def _length(n):
    """Extension bytes of a length whose nibble is 15."""
    out = bytearray()
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def lz4_sequence(literals, offset=None, match=0):
    """One sequence: the literals, then a match of ``match`` (>= 4) bytes at ``offset``; ``offset=None``: the last one."""
    ll = len(literals)
    ml = match - 4 if offset is not None else 0
    assert ml >= 0
    out = bytearray([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length(ll)
    out += literals
    if offset is not None:
        assert 1 <= offset <= 65535
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length(ml)
    return bytes(out)


class Lz4Asm:
    """A hand-assembled LZ4 block and, computed byte by byte next to it, what it decodes to."""

    def __init__(self):
        self.stream, self.out, self.pending = bytearray(), bytearray(), b""

    def lit(self, data):
        self.pending += bytes(data)
        return self

    def match(self, offset, length):
        self.stream += lz4_sequence(self.pending, offset, length)
        self.out += self.pending
        self.pending = b""
        assert offset <= len(self.out)
        for _ in range(length):
            self.out.append(self.out[-offset])
        return self

    def end(self):
        self.stream += lz4_sequence(self.pending)
        self.out += self.pending
        self.pending = b""
        return bytes(self.stream), bytes(self.out)


def _common(data, a, b, limit):
    """Length of the common prefix of data[a:] and data[b:] (b > a, the ranges may overlap), at most ``limit``."""
    m = 0
    while m < limit:
        step = min(64, limit - m, b - a)  # (never compare bytes the match itself would produce out of order)
        if data[a + m : a + m + step] == data[b + m : b + m + step]:
            m += step
            continue
        while data[a + m] == data[b + m]:
            m += 1
        break
    return m


def lz4_compress(data):
    """Greedy LZ4 block encoder (hash of 4 bytes -> last position, LZ4's end-of-block rules: the last match starts at
    least 12 bytes before the end and the last 5 bytes are literals)."""
    data = bytes(data)
    n = len(data)
    out, table = bytearray(), {}
    anchor = i = 0
    misses = 0
    while i < n - 12:
        key = data[i : i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > 65535:
            misses += 1
            i += 1 + (misses >> 6)
            continue
        misses = 0
        m = 4 + _common(data, cand + 4, i + 4, n - 5 - (i + 4))
        out += lz4_sequence(data[anchor:i], i - cand, m)
        i += m
        anchor = i
    out += lz4_sequence(data[anchor:])
    return bytes(out)


def lz4_decompress_py(stream, n):
    """Plain LZ4 block decoder (tests of the encoder above only)."""
    out, ip = bytearray(), 0
    while True:
        token = stream[ip]
        ip += 1
        ll = token >> 4
        if ll == 15:
            while True:
                b = stream[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        out += stream[ip : ip + ll]
        ip += ll
        if ip == len(stream):
            break
        off = stream[ip] | (stream[ip + 1] << 8)
        ip += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = stream[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        for _ in range(ml + 4):
            out.append(out[-off])
    assert len(out) == n
    return bytes(out)


# ---- shuffles ------------------------------------------------------------------------------------------------------
def shuffle2(raw):
    a = np.frombuffer(raw[: len(raw) // 2 * 2], np.uint8).reshape(-1, 2)
    return a[:, 0].tobytes() + a[:, 1].tobytes() + raw[len(raw) // 2 * 2 :]


def bitshuffle2(raw):
    """c-blosc 1.21's bit shuffle of 2-byte elements: only a block whose element count is a multiple of 8 is shuffled
    (16 rows of ne / 8 bytes: row 8 s + b = bit b of byte s of every element, element 8 j + k in bit k of byte j)."""
    ne = len(raw) // 2
    if ne == 0 or ne % 8:
        return raw
    a = np.frombuffer(raw[: 2 * ne], np.uint8).reshape(ne, 2)
    rows = []
    for s in range(2):
        bits = np.unpackbits(a[:, s : s + 1], axis=1, bitorder="little")  # [element, bit]
        for b in range(8):
            rows.append(np.packbits(bits[:, b], bitorder="little").tobytes())
    return b"".join(rows) + raw[2 * ne :]


# ---- the container ---------------------------------------------------------------------------------------------------
def _zstd(data, level=3):
    from test_zstd_decoder_host import zstd_compress

    return zstd_compress(data, level)


def blosc_frame(raw, blocksize, codec=LZ4, shuffle=SHUFFLE, split=True, streams=None, compress=None):
    """A c-blosc 1.x frame of typesize 2.  ``split``: the "don't split" flag is clear, so every block but a leftover
    one holds two streams (when ``blocksize / 2 >= 128``).  A stream the codec does not make smaller is stored.
    ``streams``: {(block, stream): bytes} replaces a coded stream (hand-assembled ones; ``len == raw size`` = stored);
    ``compress``: replaces the codec's encoder."""
    n = len(raw)
    nblocks = -(-n // blocksize)
    enc = compress or (lz4_compress if codec == LZ4 else _zstd)
    table, body = [], b""
    at = 16 + 4 * nblocks
    for b in range(nblocks):
        blk = raw[b * blocksize : (b + 1) * blocksize]
        if shuffle == SHUFFLE:
            blk = shuffle2(blk)
        elif shuffle == BITSHUFFLE:
            blk = bitshuffle2(blk)
        nsplit = 2 if (split and len(blk) == blocksize and blocksize // 2 >= 128) else 1
        ne = len(blk) // nsplit
        table.append(at + len(body))
        for j in range(nsplit):
            part = blk[j * ne : (j + 1) * ne]
            if streams and (b, j) in streams:
                z = streams[(b, j)]  # as it is: a longer stream than the bytes it holds is legal, if pointless
            else:
                z = enc(part)
                if len(z) >= len(part):
                    z = part
            body += struct.pack("<I", len(z)) + z
    flags = {NOSHUFFLE: 0, SHUFFLE: 0x1, BITSHUFFLE: 0x4}[shuffle] | (0 if split else 0x10) | (codec << 5)
    hdr = struct.pack("<BBBBIII", 2, 1, flags, 2, n, blocksize, 16 + 4 * nblocks + len(body))
    return hdr + b"".join(struct.pack("<I", t) for t in table) + body


def blosclz_literals(part):
    """A blosclz stream of literal runs only (control byte c < 32: c + 1 literals follow)."""
    out = bytearray()
    for i in range(0, len(part), 32):
        run = part[i : i + 32]
        out.append(len(run) - 1)
        out += run
    return bytes(out)


def blosclz_frame(raw):
    """One unsplit, unshuffled block of blosclz literal runs: a frame the host decodes in every mode."""
    z = blosclz_literals(raw)
    body = struct.pack("<I", 20) + struct.pack("<I", len(z)) + z
    return struct.pack("<BBBBIII", 2, 1, 0x10 | (BLOSCLZ << 5), 2, len(raw), len(raw), 16 + len(body)) + body


# ---- the corpus of the CPU and GPU tests -----------------------------------------------------------------------------
def brick(seed, nbytes):
    return synth.synthetic_plane(seed, 64, 1024).tobytes()[:nbytes]


def _hand_streams():
    """name -> (LZ4 block, its bytes): the corner cases of the block format."""
    rng = np.random.default_rng(11)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    cases = {}

    def finish(asm, k):  # >= k closing literals that make the length even (2-byte elements)
        return asm.lit(noise(k + (len(asm.out) + len(asm.pending) + k) % 2)).end()

    a = Lz4Asm().lit(b"ab").match(1, 4).lit(b"cd").match(2, 19).lit(b"xyz").match(3, 18 + 255)  # 0, 1 and 2 extensions
    a.lit(noise(14)).match(1, 4 + 15 + 255 + 255 + 7).lit(noise(15)).match(7, 5).lit(noise(15 + 255)).match(300, 40)
    a.lit(noise(15 + 255 + 255 + 3)).match(1, 9000).lit(b"").match(2, 4).lit(b"").match(3, 6)
    cases["offsets 1 2 3, lengths with 0 1 and several extension bytes"] = finish(a, 20)
    far = Lz4Asm().lit(noise(65535)).match(65535, 4000).lit(noise(9)).match(65535, 70).lit(noise(7))
    cases["offset 65535"] = finish(far, 0)
    return cases


def hand_frames():
    """(name, frame, raw): unsplit, unshuffled frames around the hand-assembled LZ4 blocks (one block each), plus
    split blocks with a stored stream, streams of two representations, a leftover block, and split zstd."""
    out = []
    for name, (stream, raw) in _hand_streams().items():
        if len(raw) % 2:
            raise AssertionError(name)
        f = blosc_frame(raw, len(raw), LZ4, NOSHUFFLE, split=False, streams={(0, 0): stream})
        assert struct.unpack("<I", f[20:24])[0] == len(stream), name  # (the hand-made block is what the frame holds)
        out.append(("lz4 " + name, f, raw))
    rng = np.random.default_rng(5)
    # a block that is one literal run is longer than its bytes: it shares a split block with a stream of zeros
    lits = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    raw = lits + bytes(4096)
    f = blosc_frame(raw, 8192, LZ4, NOSHUFFLE, split=True, streams={(0, 0): lz4_sequence(lits)})
    assert struct.unpack("<I", f[20:24])[0] == 4096 + 1 + 16 + 1
    out.append(("lz4 split, one literal run + zeros", f, raw))
    # byte-shuffled noise-low / constant-high uint16: the low-byte stream is stored, the high-byte stream is coded
    v = (rng.integers(0, 256, 16384).astype(np.uint16) | 0x0300).tobytes()
    f = blosc_frame(v, 16384, LZ4, SHUFFLE, split=True)
    ne = 8192
    p0 = struct.unpack("<I", f[16:20])[0]
    l0 = struct.unpack("<I", f[p0 : p0 + 4])[0]
    l1 = struct.unpack("<I", f[p0 + 4 + l0 : p0 + 8 + l0])[0]
    assert l0 == ne and l1 < ne  # block 0: a stored stream, then an LZ4 stream
    out.append(("lz4 split, stored + coded streams", f, v))
    out.append(("zstd split, stored + coded streams", blosc_frame(v, 16384, ZSTD, SHUFFLE, split=True), v))
    # two representations inside one block: stream 0 hand-assembled (one literal run), stream 1 from the encoder
    b0 = shuffle2(brick(2, 32768))
    lit_run = lz4_sequence(b0[:16384])
    assert len(lit_run) > 16384  # ... which the container would store: use a shorter hand-made stream instead
    zeros_low = (np.arange(16384, dtype=np.uint16) // 64 * 256).astype(np.uint16).tobytes()  # low bytes 0, high a ramp
    sh = shuffle2(zeros_low)
    s0 = Lz4Asm().lit(sh[:1]).match(1, 16384 - 1 - 5).lit(sh[16379:16384]).end()[0]
    f = blosc_frame(zeros_low, 32768, LZ4, SHUFFLE, split=True, streams={(0, 0): s0})
    out.append(("lz4 split, hand-made run stream + encoder stream", f, zeros_low))
    # 3 full blocks + a leftover block (never split), byte and bit shuffle, both codecs
    big = brick(3, 3 * 16384 + 5000)
    for codec, cn in ((LZ4, "lz4"), (ZSTD, "zstd")):
        for sh_mode, sn in ((SHUFFLE, "shuffle"), (BITSHUFFLE, "bitshuffle"), (NOSHUFFLE, "noshuffle")):
            out.append(("{} split {} with a leftover block".format(cn, sn),
                        blosc_frame(big, 16384, codec, sh_mode, split=True), big))  # fmt: skip
            out.append(("{} unsplit {}".format(cn, sn), blosc_frame(big, 16384, codec, sh_mode, split=False), big))
    odd = brick(4, 40001)  # an odd tail byte in the leftover block
    out.append(("lz4 split shuffle, odd size", blosc_frame(odd, 8192, LZ4, SHUFFLE, split=True), odd))
    out.append(("lz4 split bitshuffle, odd size", blosc_frame(odd, 8192, LZ4, BITSHUFFLE, split=True), odd))
    plane = synth.synthetic_plane(6, 256, 512).tobytes()  # 256 KiB: c-blosc's block size at clevel 5
    out.append(("lz4 split shuffle 256 KiB", blosc_frame(plane, 256 * 1024, LZ4, SHUFFLE, split=True), plane))
    return out


def golden_any_frames():
    """(case string, frame, raw) of the committed c-blosc 1.21.0 frames (tests/golden/blosc_frames.npz) with LZ4 or
    LZ4HC inside and typesize 2: the frames DSX_ZDEC_ANY adds to the device's share; and the list of all the others."""
    import os

    from test_blosc import payload

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blosc_frames.npz"))
    picked, others, k = [], [], 0
    while "frame_%03d" % k in g.files:
        case = str(g["case_%03d" % k])
        f = case.split()
        raw = payload(f[4], int(f[5]), int(f[6]))
        item = (case, g["frame_%03d" % k].tobytes(), raw)
        (picked if (f[0] in ("lz4", "lz4hc") and int(f[3]) == 2) else others).append(item)
        k += 1
    return picked, others
