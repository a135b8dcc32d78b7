"""Test infrastructure for what ``DSX_ZDEC_ALL`` adds to the device decoder (``csrc/dsx_inflate.h``: zlib streams and
blosclz): a bit writer for hand-assembled DEFLATE blocks, a small greedy blosclz encoder, the corpus of zlib streams,
the malformed ones, and task tables in the style of table B of tests/zdec_cases.py.  tests/test_inflate_decoder_host.py
runs the tables through the host build (``dsx_blosc_decode_ref``), tests/test_gpu_inflate_cases.py through the kernel;
only the executor differs.  Every valid zlib stream here is first decoded with Python's ``zlib`` (``checked``)."""

import os
import struct
import zlib

import numpy as np

import blosc_any_frames as baf
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod

E = eng_mod
ZLIB = 3  # c-blosc's inner codec number (baf has LZ4, ZSTD, BLOSCLZ)
# csrc/dsx_zstd_dec.h Status
E_TRUNCATED, E_RESERVED, E_OFFSET, E_OUTPUT, E_CHECKSUM, E_CODES, E_STORED, E_HEADER = 1, 4, 11, 12, 14, 15, 16, 17


def checked(stream, data):
    """``stream`` if Python's zlib decodes it to exactly ``data``."""
    assert zlib.decompress(stream) == data
    return stream


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return checked(c.compress(data) + c.flush(), data)


# ---- hand-assembled DEFLATE ---------------------------------------------------------------------------------------------
class Bits:
    """Bits of a DEFLATE stream: values LSB first, Huffman codes starting from their most significant bit."""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, code, n):
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def raw(self, data):
        assert len(self.bits) % 8 == 0
        for b in data:
            self.put(b, 8)
        return self

    def tobytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.array(bits, np.uint8), bitorder="little").tobytes()


def canon(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (0: no code)."""
    out, code = {}, 0
    for n in range(1, 16):
        for s, ln in enumerate(lens):
            if ln == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


def fixed_codes():
    return canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canon([5] * 32)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]  # fmt: skip
DIST_BITS = [0, 0, 0, 0] + [b for b in range(1, 14) for _ in (0, 1)]


def put_symbols(w, ll, dd, symbols):
    """``symbols``: ints (literals, 256) and ("m", length, distance) / ("raw", litlen symbol) / ("rawd", length
    symbol, distance symbol) entries, coded with the sets ``ll`` / ``dd``."""
    for s in symbols:
        if isinstance(s, int):
            w.code(*ll[s])
        elif s[0] == "raw":
            w.code(*ll[s[1]])
        elif s[0] == "rawd":
            w.code(*ll[s[1]])
            w.code(*dd[s[2]])
        else:
            _, length, dist = s
            i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
            w.code(*ll[257 + i]).put(length - LEN_BASE[i], LEN_BITS[i])
            j = max(k for k in range(30) if DIST_BASE[k] <= dist)
            w.code(*dd[j]).put(dist - DIST_BASE[j], DIST_BITS[j])
    return w


def fixed_block(w, symbols, final):
    w.put(1 if final else 0, 1).put(1, 2)
    return put_symbols(w, *fixed_codes(), list(symbols) + [256])


def stored_block(w, data, final, nlen=None):
    w.put(1 if final else 0, 1).put(0, 2).align()
    w.put(len(data), 16).put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    return w.raw(data)


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_block(w, nlen, ndist, ops, symbols, final, cl_lens=None, end=True):
    """A dynamic block whose code-length sequence is ``ops``: (symbol 0 .. 15,) or (16, repeat) / (17, zeros) /
    (18, zeros); their expansion is the ``nlen + ndist`` lengths.  The code-length code is complete (zlib refuses any
    other): the used symbols get the lengths 1, 2, ..., k - 1, k - 1 unless ``cl_lens`` gives them."""
    lens = []
    for op in ops:
        if op[0] < 16:
            lens.append(op[0])
        elif op[0] == 16:
            lens += [lens[-1]] * op[1]
        else:
            lens += [0] * op[1]
    assert len(lens) == nlen + ndist, (len(lens), nlen + ndist)
    if cl_lens is None:
        used = sorted({op[0] for op in ops})
        if len(used) == 1:
            used.append((used[0] + 1) % 16)
        assert len(used) <= 8
        cl_lens = [0] * 19
        for i, s in enumerate(used):
            cl_lens[s] = min(i + 1, len(used) - 1)
    ncode = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
    ncode = max(ncode, 4)
    w.put(1 if final else 0, 1).put(2, 2).put(nlen - 257, 5).put(ndist - 1, 5).put(ncode - 4, 4)
    for i in range(ncode):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl = canon(cl_lens)
    for op in ops:
        w.code(*cl[op[0]])
        if op[0] == 16:
            w.put(op[1] - 3, 2)
        elif op[0] == 17:
            w.put(op[1] - 3, 3)
        elif op[0] == 18:
            w.put(op[1] - 11, 7)
    ll, dd = canon(lens[:nlen]), canon(lens[nlen:])
    return put_symbols(w, ll, dd, list(symbols) + ([256] if end else []))


def zlib_wrap(w, data, adler=None, header=b"\x78\x9c"):
    body = w.tobytes() if isinstance(w, Bits) else w
    return header + body + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def _lits_65_66(extra):
    """Code-length ops of a literal/length alphabet with 65 ('A'), 66 ('B'), 256 and ``extra`` = [(symbol, length)]
    behind 256; 65, 66 and 256 have 2 bits."""
    return [(18, 65), (2,), (2,), (18, 138), (18, 51), (2,)] + extra


def hand_streams():
    """[(name, zlib stream, data)]: valid streams zlib's encoder rarely or never writes."""
    out = []
    # 65, 66, 256, 257 and four distance codes, all of 2 bits: one repeat code covers 257 and the distance alphabet
    w = dynamic_block(Bits(), 258, 4, [(18, 65), (2,), (2,), (18, 138), (18, 51), (2,), (16, 5)],
                      [65, 66, 65, ("m", 3, 1), ("m", 3, 4), 66], True)  # fmt: skip
    data = b"ABA" + b"AAA" + b"AAA" + b"B"
    out.append(("repeat code over both alphabets", checked(zlib_wrap(w, data), data), data))
    # a distance set that is one code of 1 bit (incomplete, and legal)
    w = dynamic_block(Bits(), 258, 1, _lits_65_66([(2,), (1,)]), [65, 66, ("m", 3, 1), 65, ("m", 3, 1)], True)
    data = b"AB" + b"BBB" + b"A" + b"AAA"
    out.append(("single-code distance set", checked(zlib_wrap(w, data), data), data))
    # no distance code at all, no length code: literals only (65 has 1 bit, 66 and 256 two)
    w = dynamic_block(Bits(), 257, 1, [(18, 65), (1,), (2,), (18, 138), (18, 51), (2,), (0,)], [65, 66, 66, 65], True)
    data = b"ABBA"
    out.append(("dynamic block without a match", checked(zlib_wrap(w, data), data), data))
    # stored blocks of LEN = 0 before, between and behind the others
    w = Bits()
    stored_block(w, b"", False)
    stored_block(w, b"", False)
    stored_block(w, b"stored bytes", False)
    fixed_block(w, [ord("x"), ("m", 5, 1)], False)
    stored_block(w, b"", False)
    stored_block(w, b"!", False)
    stored_block(w, b"", True)
    data = b"stored bytes" + b"xxxxxx" + b"!"
    out.append(("stored blocks of LEN 0", checked(zlib_wrap(w, data), data), data))
    # distances zlib's encoder never reaches (its window is 32 768 - 262): exactly 32 768 and 32 767
    rng = np.random.default_rng(41)
    head = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = stored_block(Bits(), head, False)
    fixed_block(w, [("m", 40, 32768), ("m", 258, 32767), 7, ("m", 3, 32768)], True)
    data = bytearray(head)
    for m in ((40, 32768), (258, 32767), None, (3, 32768)):
        if m is None:
            data.append(7)
            continue
        for _ in range(m[0]):
            data.append(data[-m[1]])
    data = bytes(data)
    out.append(("distances 32768 and 32767", checked(zlib_wrap(w, data), data), data))
    # length 258 both ways: symbol 285, and symbol 284 with its extra bits at 30 (257) next to it
    w = fixed_block(Bits(), [ord("r"), ("m", 258, 1), ("m", 257, 1), ("m", 258, 259)], True)
    data = b"r" * (1 + 258 + 257 + 258)
    out.append(("lengths 258 and 257", checked(zlib_wrap(w, data), data), data))
    return out


def periodic(p, n=1500, seed=0):
    rng = np.random.default_rng(1000 + p + seed)
    unit = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
    return (unit * (n // p + 1))[:n]


def zlib_corpus():
    """[(name, zlib stream, data)]: what Python's zlib writes at the levels and strategies of the issue."""
    rng = np.random.default_rng(43)
    noise = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    inputs = {"empty": b"", "one": b"\x5a", "noise": noise, "brick": baf.shuffle2(baf.brick(11, 40000)),
              "brick unshuffled": baf.brick(12, 30000), "runs": bytes(3000) + b"\x01" * 700 + bytes(5000),
              "text": b"the quick brown fox jumps over the lazy dog. " * 300}  # fmt: skip
    strategies = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}
    out = []
    for name, data in inputs.items():
        for level in (0, 1, 6, 9):
            for sn, strat in strategies.items():
                out.append(("{} level {} {}".format(name, level, sn), deflate(data, level, strat), data))
    for p in range(1, 301):
        out.append(("period {}".format(p), deflate(periodic(p), 6 if p % 2 else 1), periodic(p)))
    parts = [baf.brick(13, 9000), noise[:3000], bytes(4000), baf.brick(14, 5000)]
    c = zlib.compressobj(6)
    z = b"".join(c.compress(p) + c.flush(zlib.Z_FULL_FLUSH) for p in parts) + c.flush(zlib.Z_FULL_FLUSH) + c.flush()
    out.append(("full flushes", checked(z, b"".join(parts)), b"".join(parts)))
    big = baf.brick(15, 65536) + baf.shuffle2(baf.brick(16, 65536)) + noise + bytes(70000)  # several dynamic blocks
    out.append(("several blocks", deflate(big, 6), big))
    return out


def zlib_table(streams, flag=0):
    t = zc.Table()
    for i, (name, z, data) in enumerate(streams):
        t.add(name, z, len(data), E.TASK_ZLIB | flag, zc.decoded_form(data, flag), dst_res=i % 16, src_res=i % 4)
    return t


def malformed_streams():
    """[(name, bytes, dst_len, documented status or None)].  Every entry is refused by ``zlib.decompress`` or yields
    another length than ``dst_len`` (``zlib_rejects``)."""
    out = []
    data = b"ABA" + b"AAA" + b"AAA" + b"B"
    good = hand_streams()[0][1]
    brick = baf.brick(17, 3000)
    for tag, z, d in (("hand", good, data), ("level 6", deflate(brick, 6), brick), ("fixed", deflate(brick[:200], 6, zlib.Z_FIXED), brick[:200]),
                      ("stored", deflate(brick[:300], 0), brick[:300])):  # fmt: skip
        cuts = range(len(z)) if len(z) < 80 else sorted(set(range(0, len(z), max(1, len(z) // 97))) | set(range(len(z) - 12, len(z))))
        for cut in cuts:
            out.append(("{} cut at byte {}".format(tag, cut), z[:cut], len(d), E_TRUNCATED if cut >= 2 else None))
        out.append((tag + " one byte too many for dst_len", z, len(d) - 1, E_OUTPUT))
        out.append((tag + " one byte too few for dst_len", z, len(d) + 1, E_OUTPUT))
        bad = bytearray(z)
        bad[-1] ^= 0x01
        out.append((tag + " wrong Adler-32", bytes(bad), len(d), E_CHECKSUM))
        out.append((tag + " FDICT set", bytes([0x78, 0xBB]) + z[2:], len(d), E_HEADER))
        out.append((tag + " method 7", bytes([0x77, 0x9D]) + z[2:], len(d), E_HEADER))
        out.append((tag + " FCHECK wrong", bytes([0x78, 0x9D]) + z[2:], len(d), E_HEADER))
    out.append(("window of 64 KiB", bytes([0x88, 0x1C]) + good[2:], len(data), E_HEADER))
    one = lambda w, d=b"": zlib_wrap(w, d)  # noqa: E731
    out.append(("BTYPE 3", one(Bits().put(1, 1).put(3, 2)), 0, E_RESERVED))
    out.append(("LEN / NLEN mismatch", one(stored_block(Bits(), b"abc", True, nlen=0xFFFD), b"abc"), 3, E_STORED))
    out.append(("stored block longer than the stream", one(Bits().put(1, 1).put(0, 2).align().put(9, 16).put(9 ^ 0xFFFF, 16).raw(b"abc")),
                9, E_TRUNCATED))  # fmt: skip
    # code sets: 65, 66 and 256 with 1 bit each (over-subscribed); 65 and 256 with 2 bits (incomplete); no 256
    over = dynamic_block(Bits(), 257, 1, [(18, 65), (1,), (1,), (18, 138), (18, 51), (1,), (0,)], [], True, end=False)
    out.append(("over-subscribed literal/length set", one(over), 0, E_CODES))
    inc = dynamic_block(Bits(), 257, 1, [(18, 65), (2,), (18, 138), (18, 52), (2,), (0,)], [], True, end=False)
    out.append(("incomplete literal/length set", one(inc), 0, E_CODES))
    incd = dynamic_block(Bits(), 257, 2, [(18, 65), (1,), (2,), (18, 138), (18, 51), (2,), (2,), (2,)], [65], True)
    out.append(("incomplete distance set", one(incd, b"A"), 1, E_CODES))
    overd = dynamic_block(Bits(), 257, 3, [(18, 65), (1,), (2,), (18, 138), (18, 51), (2,), (1,), (1,), (1,)], [65], True)
    out.append(("over-subscribed distance set", one(overd, b"A"), 1, E_CODES))
    noeob = dynamic_block(Bits(), 257, 1, [(18, 65), (1,), (1,), (18, 138), (18, 52), (0,)], [], True, end=False)
    out.append(("no end-of-block code", one(noeob), 0, E_CODES))
    cl_over = dynamic_block(Bits(), 257, 1, [(18, 65), (1,), (2,), (18, 138), (18, 51), (2,), (0,)], [65], True,
                            cl_lens=[1, 1, 1] + [0] * 15 + [2])  # fmt: skip
    out.append(("over-subscribed code-length code", one(cl_over, b"A"), 1, E_CODES))
    cl_inc = dynamic_block(Bits(), 257, 1, [(18, 65), (1,), (2,), (18, 138), (18, 51), (2,), (0,)], [65], True,
                           cl_lens=[2, 2, 2] + [0] * 15 + [3])  # fmt: skip
    out.append(("incomplete code-length code", one(cl_inc, b"A"), 1, E_CODES))
    first16 = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)  # HCLEN 4: the lengths of 16, 17, 18, 0
    first16.put(1, 3).put(0, 3).put(0, 3).put(1, 3).code(1, 1).put(0, 2)  # ... and a repeat (16) with nothing before it
    out.append(("repeat code with no previous length", one(first16), 0, E_CODES))
    over_run = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for i in range(19):  # the code-length code: 1 and 18 with 1 bit; then two zero runs of 138: more than 258 lengths
        over_run.put({18: 1, 1: 1}.get(CL_ORDER[i], 0), 3)
    over_run.code(*canon([0, 1] + [0] * 16 + [1])[18]).put(127, 7).code(*canon([0, 1] + [0] * 16 + [1])[18]).put(127, 7)
    out.append(("repeat past the two alphabets", one(over_run), 0, E_CODES))
    ll, dd = fixed_codes()
    w = put_symbols(Bits().put(1, 1).put(1, 2), ll, dd, [97, ("raw", 286)])
    out.append(("length symbol 286", one(w, b"a"), 1, E_CODES))
    w = put_symbols(Bits().put(1, 1).put(1, 2), ll, dd, [97, ("rawd", 257, 30)])
    out.append(("distance symbol 30", one(w, b"a"), 1, E_CODES))
    w = fixed_block(Bits(), [97, ("m", 3, 2)], True)
    out.append(("distance before the start", one(w, b"aaaa"), 4, E_OFFSET))
    w = fixed_block(Bits(), [("m", 3, 1)], True)
    out.append(("match as the first symbol", one(w, b"aaa"), 3, E_OFFSET))
    w = fixed_block(Bits(), [97, 98], False)
    out.append(("no final block", one(w, b"ab"), 2, None))  # (the trailer is read as a block header)
    return out


def zlib_rejects(stream, dst_len):
    try:
        return len(zlib.decompress(stream)) != dst_len
    except zlib.error:
        return True


def malformed_table():
    """Every malformed stream between good tasks, at the residues of table B; the good tasks keep their bytes."""
    t = zc.Table()
    good = [(n, z, d) for n, z, d in hand_streams() if len(z) < 200]
    for i, (name, z, n, st) in enumerate(malformed_streams()):
        g = good[i % len(good)]
        t.add("good " + g[0], g[1], len(g[2]), E.TASK_ZLIB, g[2], dst_res=(2 * i) % 16, src_res=(2 * i) % 4)
        t.add(name, z, n, E.TASK_ZLIB, None, status=st, dst_res=(2 * i + 1) % 16, src_res=(2 * i + 1) % 4)
    g = good[0]
    t.add("good " + g[0], g[1], len(g[2]), E.TASK_ZLIB, g[2])
    return t


# ---- blosclz ------------------------------------------------------------------------------------------------------------
def blosclz_match(length, dist):
    """One match instruction (csrc/dsx_inflate.h blosclz_next): length >= 3, distance 1 .. 65536 + 8191."""
    assert length >= 3 and 1 <= dist <= 65535 + 8192
    d = dist - 1
    far = d >= 8191
    low = 31 if far else d >> 8
    out = bytearray()
    if length - 2 < 7:
        out.append(((length - 2) << 5) | low)
    else:
        out.append((7 << 5) | low)
        rest = length - 9
        while rest >= 255:
            out.append(255)
            rest -= 255
        out.append(rest)
    if far:
        out += bytes([255]) + struct.pack(">H", d - 8191)
    else:
        out.append(d & 255)
    return bytes(out)


def blosclz_literals(data):
    return baf.blosclz_literals(data)


def blosclz_compress(data):
    """A greedy blosclz encoder (3-byte hash, the latest position wins).  The stream starts with a literal and, like
    c-blosc's, ends with one: the decoder wants two bytes behind the control byte of a match."""
    n = len(data)
    out, lit = bytearray(), bytearray()
    table = {}
    i = 0

    def flush():
        for k in range(0, len(lit), 32):
            run = lit[k : k + 32]
            out.append(len(run) - 1)
            out.extend(run)
        lit.clear()

    while i < n:
        key = data[i : i + 3]
        j = table.get(key) if i + 3 <= n - 2 and i > 0 else None
        table[key] = i
        if j is not None and i - j <= 65535 + 8192:
            m = 3
            limit = n - 2 - i  # the last two bytes stay literals
            while m < limit and data[j + m] == data[i + m]:
                m += 1
            flush()
            out += blosclz_match(m, i - j)
            i += m
        else:
            lit.append(data[i])
            i += 1
    flush()
    return bytes(out)


def blosclz_compress_runs(data, shortest=16):
    """A blosclz encoder for whole chunks: byte runs of ``shortest`` and more become matches of distance 1, everything
    else literal runs (found with numpy: a Python step per run, not per byte)."""
    n = len(data)
    if n < 4:
        return blosclz_literals(data)
    a = np.frombuffer(data, np.uint8)
    edges = np.concatenate(([0], np.flatnonzero(a[1:] != a[:-1]) + 1, [n]))
    starts, lengths = edges[:-1], np.diff(edges)
    out, at = bytearray(), 0
    for s0, ln in zip(starts[lengths >= shortest].tolist(), lengths[lengths >= shortest].tolist()):
        m = min(ln - 1, n - 2 - (s0 + 1))  # the first byte of the run is a literal; the last two bytes of the data too
        if m < 3:
            continue
        out += blosclz_literals(data[at : s0 + 1])
        out += blosclz_match(m, 1)
        at = s0 + 1 + m
    return bytes(out + blosclz_literals(data[at:]))


def blosclz_decompress_py(stream, n):
    """blosclz.c's decoder, byte by byte (the check of the encoder above)."""
    out = bytearray()
    ip = 0
    if not stream:
        return bytes(out)
    ctrl = stream[0] & 31
    ip = 1
    while True:
        if ctrl >= 32:
            length = (ctrl >> 5) - 1
            ofs = (ctrl & 31) << 8
            if length == 6:
                while True:
                    code = stream[ip]
                    ip += 1
                    length += code
                    if code != 255:
                        break
            code = stream[ip]
            ip += 1
            length += 3
            dist = ofs + code
            if code == 255 and ofs == 31 << 8:
                dist = (stream[ip] << 8) + stream[ip + 1] + 8191
                ip += 2
            dist += 1
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
        else:
            out += stream[ip : ip + ctrl + 1]
            ip += ctrl + 1
        if ip >= len(stream):
            break
        ctrl = stream[ip]
        ip += 1
    assert len(out) == n
    return bytes(out)


def blosclz_hand_streams():
    """[(name, stream, data)]: the corners of the format."""
    rng = np.random.default_rng(47)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    out = []

    def build(name, parts):
        stream, data = bytearray(), bytearray()
        for p in parts:
            if isinstance(p, bytes):
                stream += blosclz_literals(p)
                data += p
            else:
                stream += blosclz_match(*p)
                for _ in range(p[0]):
                    data.append(data[-p[1]])
        assert blosclz_decompress_py(bytes(stream), len(data)) == bytes(data), name
        out.append((name, bytes(stream), bytes(data)))

    build("literal runs of 1, 32 and 33", [b"a", noise(32), noise(33)])
    build("lengths 3 .. 8, 9 (one extension byte of 0), 263, 264 (255 + 0), 1000",
          [noise(40)] + [(m, 7) for m in (3, 4, 5, 6, 7, 8, 9, 10, 263, 264, 265, 1000)] + [b"zz"])  # fmt: skip
    build("overlapping matches of distance 1, 2, 3, 63, 64, 65", [noise(70)] + [x for d in (1, 2, 3, 63, 64, 65) for x in ((300, d), noise(3))])
    build("distances 256, 8191 (the last near one), 8192 (the first far one), 8193",
          [noise(9000), (20, 256), (20, 8191), (20, 8192), (20, 8193), b"end"])  # fmt: skip
    build("far distances up to 65535 + 8192", [noise(65535 + 8192), (50, 65535 + 8192), (700, 40000), b"end"])
    build("a stream longer than the window, a literal run over its edge",
          [noise(31)] + [x for _ in range(150) for x in ((5, 9), noise(int(rng.integers(1, 30))))] + [noise(32) * 3])  # fmt: skip
    return out


def blosclz_malformed():
    """[(name, bytes, dst_len, status or None)]; no stream is as long as its dst_len (a Blosc block would hold such
    a stream as stored bytes)."""
    stream = blosclz_literals(b"abcdefgh") + blosclz_match(20, 3) + blosclz_literals(b"12345")
    n = 8 + 20 + 5
    assert blosclz_decompress_py(stream, n)
    out = [("cut at {}".format(c), stream[:c], n, None) for c in range(len(stream))]
    out.append(("one byte too many for dst_len", stream, n - 1, E_OUTPUT))
    out.append(("one byte too few for dst_len", stream, n + 1, E_OUTPUT))
    out.append(("distance before the start", blosclz_literals(b"abc") + blosclz_match(5, 4) + blosclz_literals(b"xy"), 10, E_OFFSET))
    out.append(("match past the output", blosclz_literals(b"abc") + blosclz_match(200, 1) + blosclz_literals(b"xy"), 9, E_OUTPUT))
    out.append(("literals past the output", blosclz_literals(b"abcdefghijkl"), 9, E_OUTPUT))
    out.append(("a length that never ends", blosclz_literals(b"a") + bytes([0xE0]) + b"\xff" * 60, 9, None))
    out.append(("match with one byte behind its control byte", blosclz_literals(b"abcdef") + blosclz_match(4, 2), 10, E_TRUNCATED))
    out.append(("far distance cut off", blosclz_literals(b"abcdef") + blosclz_match(3, 9000)[:-1] + b"", 9, E_TRUNCATED))
    return out


# ---- table B for the new kinds -----------------------------------------------------------------------------------------
_coded = {}


def code(kind, part, alt=False):
    """``part`` as a stream of ``kind``; ``alt``: another coding (of another length)."""
    key = (kind, part, alt)
    if key not in _coded:
        if kind == E.TASK_ZLIB:
            z = deflate(part, 0 if alt else 6)
        else:
            z = blosclz_literals(part) if alt else blosclz_compress(part)
            assert blosclz_decompress_py(z, len(part)) == part
        _coded[key] = z
    return _coded[key]


def layout_table():
    """Every new kind x shuffle flag x split form at the lengths and residues of ``zdec_cases.layout_table``:
    ``(table, facts)``."""
    t, facts = zc.Table(), []
    k = [0]

    def put(name, payload, n, kind, expect, aligned):
        res = (0, 0) if aligned else (k[0] % 16, k[0] % 4)
        i = t.add(name, payload, n, kind, expect, dst_res=res[0], src_res=res[1])
        k[0] += 1
        r = t.rows[i]
        facts.append(dict(kind=kind & 0xFF, flag=kind & (E.TASK_SHUFFLE | E.TASK_BITSHUFFLE), split=bool(kind & E.TASK_SPLIT),
                          n=n, dst=r[1], src=r[0], stream=len(payload)))  # fmt: skip

    def one_length(n, aligned):
        tag = "{}{}".format(n, " aligned" if aligned else "")
        raw = zc._payload(n)
        for flag in zc.FLAGS:
            st = zc.stored_form(raw, flag)
            for codec, cn in ((E.TASK_ZLIB, "zlib"), (E.TASK_BLOSCLZ, "blosclz")):
                put("{} {:#x} {}".format(cn, flag, tag), code(codec, st), n, codec | flag, raw, aligned)
                if n % 2:
                    continue
                ne = n // 2
                halves = (st[:ne], st[ne:])
                for coded in ((1, 1), (1, 0), (0, 1), (0, 0)):
                    if ne == 0 and codec == E.TASK_BLOSCLZ and any(coded):
                        continue  # (a blosclz stream holds at least one byte)
                    parts = []
                    for h, c in zip(halves, coded):
                        z = code(codec, h) if c else h
                        if c and len(z) == ne:  # a stream as long as its share would be read as stored
                            z = code(codec, h, alt=True)
                        assert (len(z) != ne) == bool(c), (tag, len(z))
                        parts.append(struct.pack("<I", len(z)) + z)
                    put("{} split{} {:#x} {}".format(cn, coded, flag, tag), b"".join(parts), n,
                        codec | flag | E.TASK_SPLIT, raw, aligned)  # fmt: skip

    for n in zc.LENGTHS:
        one_length(n, False)
    for n in zc.ALIGNED_LENGTHS:
        one_length(n, True)
    return t, facts


def big_block_table():
    """One 256 KiB block per codec (c-blosc's block size at clevel 5), byte-shuffled."""
    from aind_smartspim_destripe_amd import synth

    plane = synth.synthetic_plane(6, 256, 512).tobytes()
    st = baf.shuffle2(plane)
    t = zc.Table()
    for codec, cn in ((E.TASK_ZLIB, "zlib"), (E.TASK_BLOSCLZ, "blosclz")):
        t.add(cn + " 256 KiB", code(codec, st), len(plane), codec | E.TASK_SHUFFLE, plane)
    return t


# ---- frames -------------------------------------------------------------------------------------------------------------
def blosc_frame(raw, blocksize, codec, shuffle=baf.SHUFFLE, split=True, level=5, runs_only=False):
    """``baf.blosc_frame`` with zlib (``ZLIB``) or blosclz (``baf.BLOSCLZ``) inside; ``runs_only``: the blosclz
    encoder for whole chunks."""
    enc = (lambda part: zlib.compress(part, level)) if codec == ZLIB else (blosclz_compress_runs if runs_only else blosclz_compress)
    return baf.blosc_frame(raw, blocksize, codec, shuffle, split, compress=enc)


def golden_all_frames():
    """(case string, frame, raw) of tests/golden/blosc_all_frames.npz (c-blosc 1.21.0, tools/make_golden_blosc_all.py)."""
    from test_blosc import payload

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blosc_all_frames.npz"))
    assert str(g["blosc_version"]) == "1.21.0"
    out, k = [], 0
    while "frame_%03d" % k in g.files:
        case = str(g["case_%03d" % k])
        f = case.split()
        out.append((case, g["frame_%03d" % k].tobytes(), payload(f[4], int(f[5]), int(f[6]))))
        k += 1
    return out
