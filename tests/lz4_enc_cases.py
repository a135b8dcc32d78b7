"""One case table for the Blosc-LZ4 encoder (``csrc/dsx_lz4_enc.h``), shared by tests/test_lz4_encoder_host.py (the
host build) and tests/test_gpu_device_codec_lz4.py (the kernel), with an independent reader of what it writes: the
c-blosc 1.x container with split streams, an LZ4 block decoder and a walker over the sequences of a block, all pure
Python.

Every case is ``(name, chunks)``: ``chunks`` a uint16 array ``[n, elements]`` -- n chunks of one size, one call of the
encoder.  A chunk is built from its two byte planes (``planes(low, high)``): the planes are the streams of a split
block.  The cases named for a length or a position place copies of a random head between random filler; with a table
of 4 096 entries a filler byte now and then takes the head's table entry, so their seeds were chosen once, for the
finder of the header (64 positions per step, 4 096 entries), and ``expectations`` says per case what a frame must
show -- a changed finder may need other seeds, never other expectations."""

import struct

import numpy as np

MEMCPYED, SHUFFLE, DONT_SPLIT, LZ4 = 0x2, 0x1, 0x10, 1
BLOCK = 256 * 1024


def planes(low, high):
    """uint16 chunk whose byte-shuffled Blosc block is the bytes ``low`` then the bytes ``high``."""
    return np.asarray(low, np.uint16) | (np.asarray(high, np.uint16) << 8)


def _periodic(rs, period, n):
    return np.resize(rs.randint(0, 256, period), n).astype(np.uint8)


def _placed(rs, n, lit, match, head=300, first=280):
    """A stream of n bytes: a random head, its first `first` bytes again (a match), `lit` random bytes, the first
    `match` bytes of the head again, random bytes.  Every copy is followed by a byte that ends it.  (The second copy is
    matched against the first, the latest position of its key: `first` >= `match`.)"""
    r = rs.randint(0, 256, head).astype(np.uint8)
    out = [r, r[:first]]
    f = rs.randint(0, 256, lit).astype(np.uint8)
    f[0] = r[first] ^ 0xFF
    out += [f, r[:match]]
    t = rs.randint(0, 256, n - head - first - lit - match).astype(np.uint8)
    t[0] = r[match] ^ 0xFF
    return np.concatenate(out + [t])


LATE_N, LATE_ZEROS = 1024, 800


def _late_repeat(rs, back, length):
    """A stream of LATE_N bytes that stays coded and ends in a repeat the finder must leave alone: LATE_ZEROS zeros (one
    match of offset 1, which ends there), random bytes, then `length` of those random bytes again from `back` bytes
    before the end -- a repeat of 4 bytes or more that ends 5 bytes before the end at the latest and would be a legal
    match but for its start within the last 12 bytes --, and random last bytes.  All bytes behind the zeros are last
    literals."""
    assert 9 <= back <= 12 and 4 <= length <= back - 5
    s = np.concatenate([np.zeros(LATE_ZEROS, np.uint8), rs.randint(1, 256, LATE_N - LATE_ZEROS).astype(np.uint8)])
    s[LATE_N - back : LATE_N - back + length] = s[LATE_ZEROS + 50 : LATE_ZEROS + 50 + length]
    return s


def length_case(lit, match, seed):
    rs = np.random.RandomState(seed)
    return planes(_placed(rs, 1400, lit, match), rs.randint(0, 256, 1400))[None]


LENGTH_CASES = ((14, 18, 0), (15, 19, 0), (269, 273, 0), (270, 274, 0))  # literals, match bytes, seed


def cases():
    rs = np.random.RandomState(2024)
    N = 20000
    noise = lambda n: rs.randint(0, 256, n).astype(np.uint8)  # noqa: E731
    zeros = lambda n: np.zeros(n, np.uint8)  # noqa: E731
    out = [
        ("empty", np.zeros((1, 0), np.uint16)),
        ("one element", np.full((2, 1), 0x1234, np.uint16)),
        ("40 elements", rs.randint(0, 3, (3, 40)).astype(np.uint16)),
        ("unsplit chunk of 128 ... 254 bytes", np.zeros((2, 100), np.uint16)),
        ("full block + 2-byte leftover", np.stack([planes(zeros(131073), np.full(131073, 7)),
                                                   planes(noise(131073) & 3, zeros(131073))])),
        ("full block + 4094-byte leftover", np.stack([planes(zeros(133119), np.full(133119, 7)),
                                                      planes(noise(133119) & 3, np.arange(133119) >> 12)])),
        ("short chunk that splits", np.stack([planes(_periodic(rs, 11, 70001), zeros(70001)),
                                              planes(noise(70001) & 15, np.arange(70001) >> 9)])),
        ("zeros", np.zeros((2, N), np.uint16)),
        ("noisy low, constant high", planes(noise(N), np.full(N, 9))[None]),
        ("constant low, noisy high", planes(np.full(N, 9), noise(N))[None]),
        ("noise", rs.randint(0, 65536, (2, N)).astype(np.uint16)),
        ("one full block of noise and zeros", np.stack([planes(noise(131072), zeros(131072)),
                                                        planes(zeros(131072), noise(131072))])),
    ]
    # (a frame of 2-byte elements has no stream of 13 bytes: 12 and 14 here, 13 in test_lz4_encoder_host.py)
    out.append(("full block + 12-byte leftover stream", planes(noise(131078) & 1, zeros(131078))[None]))
    out.append(("full block + 14-byte leftover stream", planes(noise(131079) & 1, zeros(131079))[None]))
    for p in (1, 2, 3, 5, 7, 13, 63, 64, 65, 100):
        out.append(("period {}".format(p), planes(_periodic(rs, p, N), _periodic(rs, p, N))[None]))
    for p in (65535, 65536, 65537):
        # (a table of 4 096 entries does not keep a position over 65 535 others: the period is 64 random bytes and
        #  zeros, which one match of offset 1 covers without an entry, so the head is still in the table when it returns)
        s = np.resize(np.concatenate([rs.randint(1, 256, 64).astype(np.uint8), zeros(p - 64)]), 70001)
        out.append(("period {}".format(p), planes(s, s)[None]))
    for lit, match, seed in LENGTH_CASES:
        out.append(("{} literals, match of {}".format(lit, match), length_case(lit, match, seed)))
    # positions
    out.append(("match into the last 5 bytes", planes(_periodic(rs, 9, 1000), zeros(1000))[None]))
    out.append(("repeat within the last 12 bytes", planes(_late_repeat(rs, 12, 7), _late_repeat(rs, 9, 4))[None]))
    mid = np.concatenate([noise(100), zeros(924)])
    out.append(("run from the middle of a group", planes(mid, np.roll(mid, 13))[None]))
    return out


def image_bricks(n=2):
    """The bricks the zstd encoder tests use: synthetic planes folded into (64, 128, 128)."""
    from aind_smartspim_destripe_amd import synth

    return np.stack([synth.synthetic_plane(k, 256, 4096).reshape(-1) for k in range(n)])


# ---- an independent reader -----------------------------------------------------------------------------------------
def lz4_sequences(block):
    """The sequences of one LZ4 block: ``[(literal length, offset, match length)]``, the last one ``(literals, 0, 0)``.
    Asserts the syntax: chained lengths, a last sequence of literals only that ends the block."""
    seqs, i, n = [], 0, len(block)
    while True:
        assert i < n, "block ends between sequences"
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        assert i <= n
        if i == n:
            assert tok & 15 == 0, "the last sequence carries a match length"
            seqs.append((lit, 0, 0))
            return seqs
        off = block[i] | (block[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        seqs.append((lit, off, ml + 4))


def lz4_block_decode(block, n):
    """One LZ4 block -> ``n`` bytes."""
    out = bytearray()
    i = 0
    for lit, off, ml in lz4_sequences(block):
        i += 1 + (0 if lit < 15 else (lit - 15) // 255 + 1)
        out += block[i : i + lit]
        i += lit
        if not ml:
            break
        assert 1 <= off <= len(out), "offset reaches in front of the block"
        i += 2 + (0 if ml - 4 < 15 else (ml - 4 - 15) // 255 + 1)
        if off >= ml:
            out += out[len(out) - off : len(out) - off + ml]
        else:
            pat = bytes(out[-off:])
            out += (pat * (ml // off + 1))[:ml]
    assert len(out) == n, (len(out), n)
    return bytes(out)


def check_stream_rules(block, n):
    """The rules a coded stream of n bytes is held to (LZ4 block format, "end of block" conditions)."""
    seqs = lz4_sequences(block)
    assert len(block) < n, "a coded stream is shorter than its bytes"
    at = 0
    for lit, off, ml in seqs[:-1]:
        at += lit
        assert 1 <= off <= 65535 and off <= at
        assert ml >= 4
        assert at < n - 12, "a match starts within the last 12 bytes"
        at += ml
        assert at <= n - 5, "a match runs into the last 5 bytes"
    assert seqs[-1][0] >= 5 or n < 13
    assert at + seqs[-1][0] == n
    if n < 13:
        assert len(seqs) == 1
    return seqs


def frame_streams(frame):
    """The streams of one frame of the writer: ``(header fields, [(block, stream index, stream bytes, data)])``; the
    header is held to section 2 of the container rules."""
    version, vlz, flags, typesize, nbytes, blocksize, cbytes = struct.unpack("<BBBBIII", frame[:16])
    assert (version, vlz, typesize, cbytes) == (2, 1, 2, len(frame))
    assert flags & ~MEMCPYED == SHUFFLE | (LZ4 << 5), flags  # byte shuffle, LZ4, "don't split" clear
    assert len(frame) <= nbytes + 16
    head = {"nbytes": nbytes, "blocksize": blocksize, "memcpyed": bool(flags & MEMCPYED)}
    if flags & MEMCPYED:
        assert len(frame) == nbytes + 16
        return head, []
    assert nbytes >= 128 and len(frame) < nbytes + 16
    assert blocksize == min(nbytes, BLOCK)
    streams = []
    end = 16 + 4 * -(-nbytes // blocksize)
    for b in range(-(-nbytes // blocksize)):
        bsize = min(blocksize, nbytes - b * blocksize)
        nsplits = 2 if bsize == blocksize and blocksize // 2 >= 128 else 1
        pos = struct.unpack("<i", frame[16 + 4 * b : 20 + 4 * b])[0]
        assert pos == end, "streams are packed back to back"
        for j in range(nsplits):
            cs = struct.unpack("<i", frame[pos : pos + 4])[0]
            assert 0 < cs <= bsize // nsplits
            streams.append((b, j, bsize // nsplits, frame[pos + 4 : pos + 4 + cs]))
            pos += 4 + cs
        end = pos
    assert end == len(frame)
    return head, streams


def py_frame_read(frame):
    """One frame -> the chunk's bytes, with the reader above."""
    head, streams = frame_streams(frame)
    if head["memcpyed"]:
        return frame[16:]
    out, blk, last = b"", b"", 0
    for b, _, n, data in streams + [(None, 0, 0, b"")]:
        if b != last:
            out += np.frombuffer(blk, np.uint8).reshape(2, -1).T.tobytes()
            blk, last = b"", b
        blk += data if len(data) == n else lz4_block_decode(data, n)
    return out


def observations(frame):
    """What the frames of a case show, for ``expectations``: a set of words."""
    head, streams = frame_streams(frame)
    seen = {"memcpyed"} if head["memcpyed"] else set()
    per_block = {}
    for b, j, n, data in streams:
        per_block.setdefault(b, []).append(len(data) == n)
        if len(data) == n:
            seen.add("stored stream")
            continue
        seen.add("coded stream")
        seqs = check_stream_rules(data, n)
        for k, (lit, off, ml) in enumerate(seqs[:-1]):
            seen |= {("literals", lit), ("match", ml), ("offset", off)}
            if k and lit >= 64:
                seen.add("unmatched group behind a match")
            if off < 64:
                seen.add("offset below 64")
            if lit >= 15 or ml - 4 >= 15:
                seen.add("chained length")
        seen.add(("last literals", seqs[-1][0]))
        if len(seqs) > 1 and seqs[-1][0] == 5:
            seen.add("match to 5 bytes before the end")
        if len(seqs) > 1:
            seen.add("match")
    for b, stored in per_block.items():
        if len(stored) == 1:
            seen.add("one-stream block")
        elif stored[0] != stored[1]:
            seen.add("stored next to coded")
    return seen


def expectations(name):
    """What at least one frame of the case must show (``observations``); ``!`` in front: what none may show;
    ``("every", key, value)``: ``(key, value)`` is shown and ``(key, x)`` for no other x."""
    table = {
        "empty": ["memcpyed"], "one element": ["memcpyed"], "40 elements": ["memcpyed"],
        "unsplit chunk of 128 ... 254 bytes": ["one-stream block", "coded stream"],
        "full block + 2-byte leftover": ["one-stream block", "stored stream", "coded stream"],
        "full block + 4094-byte leftover": ["one-stream block", "coded stream"],
        "full block + 12-byte leftover stream": ["one-stream block", "stored stream"],
        "full block + 14-byte leftover stream": ["one-stream block", "stored stream"],
        "short chunk that splits": ["coded stream", "!one-stream block"],
        "zeros": ["match to 5 bytes before the end", "chained length", ("offset", 1)],
        "noisy low, constant high": ["stored next to coded"],
        "constant low, noisy high": ["stored next to coded"],
        "noise": ["memcpyed"],
        "one full block of noise and zeros": ["stored next to coded", "!one-stream block"],
        "period 65535": [("offset", 65535), "!unmatched group behind a match"],
        "period 65536": ["unmatched group behind a match", ("offset", 1)],  # (the head's return is out of reach)
        "period 65537": ["unmatched group behind a match", ("offset", 1)],
        "match into the last 5 bytes": ["match to 5 bytes before the end"],
        # (both streams coded, and in each all that follows the zeros is literals: the repeat was not taken)
        "repeat within the last 12 bytes": ["coded stream", "!stored stream", "match", ("offset", 1),
                                            ("every", "last literals", LATE_N - LATE_ZEROS)],
        # (look-ups come before entries, so a position never finds one of its own group: an offset below 64 is seen
        #  behind a cursor move -- a group that starts less than 64 behind an entered position, as after a match --
        #  or through a run at offset 1, and that is what this case and the short periods show)
        "run from the middle of a group": [("offset", 1), "offset below 64"],
    }
    for p in (1, 2, 3, 5, 7, 13, 63, 64, 65, 100):
        table["period {}".format(p)] = [("offset", p), "chained length"] + (["offset below 64"] if p < 64 else [])
    for lit, match, _ in LENGTH_CASES:
        table["{} literals, match of {}".format(lit, match)] = [("literals", lit), ("match", match)] + (
            ["chained length"] if lit >= 15 or match >= 19 else [])
    return table[name]


def check_expectations(name, frames, offsets):
    seen = set()
    for i in range(len(offsets) - 1):
        seen |= observations(frames[offsets[i] : offsets[i + 1]])
    for want in expectations(name):
        if isinstance(want, str) and want.startswith("!"):
            assert want[1:] not in seen, (name, want)
        elif want[0] == "every":  # ("every", key, value): every (key, x) seen has x == value, and one is seen
            assert {x[1] for x in seen if isinstance(x, tuple) and x[0] == want[1]} == {want[2]}, (name, want)
        else:
            assert want in seen, (name, want, sorted(map(str, seen))[:40])
    return seen
