"""Task tables that hold the decoder of the device path (``k_zdec``, ``csrc/dsx_zdec_kernels.h``) and its host build
(``dsx_blosc_decode_ref``) to bytes no decoder of this project made: what libzstd or the LZ4 encoder of the tests was
given, a fill value.  tests/test_zdec_cases_host.py runs the tables through the host build, tests/test_gpu_zdec_cases.py
through the kernel; only the executor differs.

  A  ``mode_frames()``: the zstd corpus of tests/test_zstd_decoder_host.py, periodic buffers (one overlapping match of
     a chosen offset each), buffers for the cases only the device driver has, the hand-assembled frames; as bare zstd
     tasks of one table (``mode_table``), plain, byte-shuffled and bit-shuffled.  ``coverage()`` proves from the frames
     (``_walk`` and the ``stats`` walker of tests/host/zstd_dec_check.cpp) that every path was asked for.
  B  ``layout_table()``: every kind x flag x split form at lengths and alignments a chunk map never produces, each
     output between canary bytes.
  C  ``malformed_table()``: a fixed list of broken zstd tasks between good ones.

Every output buffer is pre-filled with ``pattern()``; ``check()`` compares the task ranges with the expectations and
every other byte with the pattern."""

import ctypes
import os
import re
import struct
import subprocess
import time

import numpy as np

import blosc_any_frames as baf
import test_zstd_decoder_host as zh
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(os.path.dirname(HERE), "aind_smartspim_destripe_amd", "csrc", "dsx_zdec_kernels.h")
GAP = 64  # untouched bytes between neighbouring outputs (at least)


def kernel_constants():
    """kSeqBatch, kLitWin, kLz4Win as the kernel header states them."""
    text = open(KERNELS).read()
    out = {}
    for name in ("kSeqBatch", "kLitWin", "kLz4Win"):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, name
        out[name] = int(m.group(1))
    return out


# ---- the shuffles and their inverses -----------------------------------------------------------------------------------
def unshuffle2(buf):
    """Inverse of ``baf.shuffle2``: n // 2 low bytes, n // 2 high bytes, an odd tail byte -> 2-byte elements."""
    ne = len(buf) // 2
    a = np.frombuffer(buf[: 2 * ne], np.uint8).reshape(2, ne)
    return a.T.tobytes() + buf[2 * ne :]


def unbitshuffle2(buf):
    """Inverse of ``baf.bitshuffle2``: 16 rows of ne / 8 bytes (row 8 s + b: bit b of byte s of every element) -> the
    elements; a buffer whose element count is 0 or not a multiple of 8 is as it is."""
    ne = len(buf) // 2
    if ne == 0 or ne % 8:
        return buf
    rows = np.frombuffer(buf[: 2 * ne], np.uint8).reshape(2, 8, ne // 8)  # [byte of the element, bit, element / 8]
    bits = np.unpackbits(rows, axis=2, bitorder="little")  # [byte, bit, element]
    elems = np.packbits(bits.transpose(2, 0, 1), axis=2, bitorder="little")  # [element, byte, 1]
    return elems.reshape(ne, 2).tobytes() + buf[2 * ne :]


FLAGS = (0, eng_mod.TASK_SHUFFLE, eng_mod.TASK_BITSHUFFLE)


def stored_form(raw, flag):
    """What a block holds for the bytes ``raw`` under a task flag (the forward shuffle)."""
    if flag == eng_mod.TASK_SHUFFLE:
        return baf.shuffle2(raw)
    if flag == eng_mod.TASK_BITSHUFFLE:
        return baf.bitshuffle2(raw)
    return raw


def decoded_form(stored, flag):
    """What a task with ``flag`` makes of a block that holds ``stored`` (the inverse shuffles, in numpy)."""
    if flag == eng_mod.TASK_SHUFFLE:
        return unshuffle2(stored)
    if flag == eng_mod.TASK_BITSHUFFLE:
        return unbitshuffle2(stored)
    return stored


# ---- tables ------------------------------------------------------------------------------------------------------------
def pattern(n):
    return ((131 * np.arange(n, dtype=np.int64) + 7) & 0xFF).astype(np.uint8)


class Table:
    """Tasks of one launch: the packed bytes, the task rows and, per task, a name, the expected status (None: the
    host build's) and the expected bytes (None: unspecified, the task fails)."""

    def __init__(self):
        self.packed = bytearray()
        self.rows, self.names, self.expect, self.status = [], [], [], []
        self.end = 0

    def add(self, name, payload, dst_len, kind, expect, status=0, dst_res=0, src_res=0, fill=None):
        if fill is None:
            self.packed += bytes((src_res - len(self.packed)) % 4)
            src = len(self.packed)
            self.packed += payload
            src_len = len(payload)
        else:
            src, src_len = fill, 0
        dst = self.end + GAP
        dst += (dst_res - dst) % 16
        self.end = dst + dst_len
        assert expect is None or len(expect) == dst_len, name
        self.rows.append((src, dst, src_len, dst_len, kind, len(self.rows)))
        self.names.append(name)
        self.expect.append(expect)
        self.status.append(status)
        return len(self.rows) - 1

    @property
    def out_bytes(self):
        return self.end + GAP

    def arrays(self):
        tasks = np.zeros(len(self.rows), eng_mod.TASK_DTYPE)
        for i, r in enumerate(self.rows):
            tasks[i] = r
        return np.frombuffer(bytes(self.packed) or b"\0", np.uint8), tasks


def run_ref(table):
    """The table through ``dsx_blosc_decode_ref`` into a pre-filled output: ``(out, status)``."""
    lib = eng_mod.load_library()
    packed, tasks = table.arrays()
    out = pattern(table.out_bytes)
    status = np.full(len(tasks), -1, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.dsx_blosc_decode_ref(vp(packed), packed.nbytes, vp(tasks), len(tasks), vp(out), out.nbytes, vp(status))
    assert rc == 0
    return out, status


LAUNCH_SECONDS = []  # (tasks, wall seconds) of every launch of run_device


def run_device(e, table):
    """The table through ``dsx_blosc_decode_device`` (one launch) into a pre-filled output: ``(out, status)``."""
    packed, tasks = table.arrays()
    n = len(tasks)
    bufs = [e.alloc(packed.nbytes), e.alloc(tasks.nbytes), e.alloc(table.out_bytes), e.alloc(4 * n)]
    d_packed, d_tasks, d_out, d_status = bufs
    try:
        d_packed.upload(packed)
        d_tasks.upload(tasks.view(np.uint8))
        d_out.upload(pattern(table.out_bytes))
        d_status.upload(np.full(n, -1, np.int32))
        e.sync()
        t0 = time.perf_counter()
        e.blosc_decode_device(d_packed, packed.nbytes, d_tasks, n, d_out, d_status, out_bytes=table.out_bytes)
        e.sync()
        LAUNCH_SECONDS.append((n, time.perf_counter() - t0))
        return d_out.download((table.out_bytes,), np.uint8), d_status.download((n,), np.int32)
    finally:
        for b in bufs:
            b.free()


def check(table, out, status, who):
    """Statuses as expected; each good task's range holds its expectation; no byte outside the ranges changed."""
    want_st = table.status
    bad = [(table.names[i], int(status[i]), want_st[i]) for i in range(len(want_st))
           if want_st[i] is not None and int(status[i]) != want_st[i]]  # fmt: skip
    assert not bad, (who, len(bad), bad[:8])
    outside = np.ones(table.out_bytes, bool)
    wrong = []
    for i, (r, exp) in enumerate(zip(table.rows, table.expect)):
        dst, n = r[1], r[3]
        outside[dst : dst + n] = False
        if exp is not None and out[dst : dst + n].tobytes() != exp:
            got = out[dst : dst + n]
            first = int(np.flatnonzero(got != np.frombuffer(exp, np.uint8))[0])
            wrong.append((table.names[i], "first wrong byte", first, "of", n))
    assert not wrong, (who, len(wrong), wrong[:8])
    touched = np.flatnonzero(outside & (out != pattern(table.out_bytes)))
    assert touched.size == 0, (who, "bytes outside every task changed", touched[:8].tolist())


# ---- A: the zstd modes -------------------------------------------------------------------------------------------------
PERIODS = (1, 2, 3, 5, 7, 13, 63, 64, 65, 100)


def periodic_data():
    """5000 bytes of period p: libzstd writes raw literals and one overlapping match of offset p."""
    rng = np.random.default_rng(23)
    out = {}
    for p in PERIODS:
        unit = rng.permutation(256)[:p].astype(np.uint8).tobytes()  # p different bytes: no shorter period
        out["period{}".format(p)] = (unit * (5000 // p + 1))[:5000]
    return out


def driver_data():
    """Buffers for cases of the device driver that the corpus may lack: a match whose source lies in the match of the
    sequence before it (and not in its own literals), and Treeless literals in a later block."""
    rng = np.random.default_rng(29)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    # "A B A' A'": A' = the tail of A; the second A' is a match into the first one with no literals between them ...
    parts = []
    for _ in range(40):
        a = noise(200)
        parts += [a, noise(7), a[40:], a[60:], noise(5)]
    chained = b"".join(parts)
    # ... and skewed literals over several blocks (one Huffman table serves later blocks)
    skew = rng.choice(np.arange(16, dtype=np.uint8), 400_000, p=np.arange(16, 0, -1) / 136.0).tobytes()
    return {"chained": chained, "skewed": skew}


def mode_frames(with_corpus=True):
    """(name, frame, data) of section A."""
    out = list(zh.corpus_frames()) if with_corpus else []
    for name, data in periodic_data().items():
        for lv in (1, 19):
            out.append(("{}@{}".format(name, lv), zh.zstd_compress(data, lv), data))
    for name, data in driver_data().items():
        for lv in (1, 3, 19):
            out.append(("{}@{}".format(name, lv), zh.zstd_compress(data, lv), data))
    out.append(("hand",) + zh._hand_frame())
    out.append(("hand fcs8",) + zh._hand_frame_fcs8())
    return out


def mode_table(frames, flag):
    """Every frame as one bare zstd task with ``flag``; the expectation is the numpy inverse shuffle of the data."""
    t = Table()
    for name, frame, data in frames:
        t.add(name, frame, len(data), eng_mod.TASK_ZSTD | flag, decoded_form(data, flag))
    return t


def build_check_exe(path, sanitize=False, source="zstd_dec_check.cpp"):
    """g++ build of a stand-alone check program of tests/host: ``zstd_dec_check.cpp`` (bare frames, the stats walker) or
    ``zdec_task_check.cpp`` (tasks of every kind); ``sanitize``: under ASan / UBSan."""
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", path, os.path.join(HERE, "host", source)], check=True)
    return path


def build_task_exe(tmp_path_factory, sanitize=False):
    return build_check_exe(str(tmp_path_factory.mktemp("zdec_task") / "zdec_task_check"), sanitize, "zdec_task_check.cpp")


def write_records(path, recs):
    """The records file of a check program: ``(frame, output bytes)`` each for ``zstd_dec_check``, ``(task bytes,
    output bytes, kind)`` for ``zdec_task_check``."""
    with open(path, "wb") as f:
        for data, *words in recs:
            f.write(struct.pack("<{}I".format(1 + len(words)), len(data), *words))
            f.write(data)


def frame_stats(exe, tmp_path, frames):
    """[{name: count}] per frame from ``zstd_dec_check stats`` (batches of kSeqBatch sequences)."""
    rec = str(tmp_path / "stats_rec.bin")
    write_records(rec, [(f, len(d)) for _, f, d in frames])
    r = subprocess.run([exe, "stats", rec, str(kernel_constants()["kSeqBatch"])], check=True, capture_output=True,
                       text=True)  # fmt: skip
    lines = r.stdout.strip().splitlines()
    names = lines[0].split()
    assert len(lines) == 1 + len(frames)
    return [dict(zip(names, map(int, ln.split()))) for ln in lines[1:]]


def _huf_streams(frame):
    """Compressed bytes of every Huffman literal stream of a frame, the four of a 4-stream section read from its
    jump table: [(block index, literal type, [stream bytes])]."""
    out = []
    d = frame[4]
    single, fcs_flag = (d >> 5) & 1, d >> 6
    p = 5 + (0 if single else 1) + {0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fcs_flag]
    k = 0
    while True:
        bh = int.from_bytes(frame[p : p + 3], "little")
        last, btype, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        if btype == 2:
            b = frame[p : p + bs]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt >= 2:
                hdr = {0: 3, 1: 3, 2: 4, 3: 5}[sf]
                v = int.from_bytes(b[:hdr], "little")
                size = {3: (v >> 14) & 0x3FF, 4: (v >> 18) & 0x3FFF, 5: (v >> 22) & 0x3FFFF}[hdr]
                tree = 0
                if lt == 2:
                    hb = b[hdr]
                    tree = 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
                if sf == 0:
                    lens = [size - tree]
                else:
                    j = hdr + tree
                    l0, l1, l2 = struct.unpack("<HHH", b[j : j + 6])
                    lens = [l0, l1, l2, size - tree - 6 - l0 - l1 - l2]
                out.append((k, lt, lens))
            p += bs
        else:
            p += bs if btype == 0 else 1
        k += 1
        if last:
            return out


def coverage(frames, stats):
    """{case: [names of frames that have it]} over section A's frames: the modes of ``_walk`` and the cases only
    the device driver has; ``missing_cases`` lists the cases without a frame."""
    k = kernel_constants()
    cov = {}

    def hit(case, name):
        cov.setdefault(case, []).append(name)

    for (name, frame, data), s in zip(frames, stats):
        assert s["status"] == 0, (name, s)
        for c in zh._walk(frame):
            hit(c, name)
        streams = _huf_streams(frame)
        assert max([0] + [x for _, _, lens in streams for x in lens]) == s["max_stream"], name  # the two walkers agree
        multi = s["blocks"] > 1
        facts = {
            "block with more than kSeqBatch sequences": s["max_seq"] > k["kSeqBatch"],
            "Huffman stream longer than kLitWin": any(x > k["kLitWin"] for _, _, lens in streams for x in lens),
            "Huffman literals, 1 stream": s["huf1"] > 0,
            "Huffman literals, 4 streams": s["huf4"] > 0,
            "Treeless literals in a later block": s["treeless_later"] > 0,
            "more than one compressed block": s["comp_blocks"] > 1,
            "Raw block in a multi-block frame": multi and s["raw_blocks"] > 0,
            "RLE block in a multi-block frame": multi and s["rle_blocks"] > 0,
            "no content size": frame[4] >> 6 == 0 and not (frame[4] >> 5) & 1,
            "output of 0 bytes": len(data) == 0,
            "output of 1 byte": len(data) == 1,
            "match with off >= ml": s["off_ge_ml"] > 0,
            "match with off < ml, off divides 64": s["pat_div"] > 0,
            "match with off < ml, off does not divide 64": s["pat_nodiv"] > 0,
            "off = 1": s["off1"] > 0,
            "barrier: source in the sequence's own literals": s["bar_own_lit"] > 0,
            "barrier: source in the match before, not in own literals": s["bar_prev_match"] > 0,
            "run of sequences without a barrier": s["max_free_run"] >= 2,
            "repeat offset": s["repeat"] > 0,
        }
        for p in PERIODS:  # the periodic buffers do what they are there for: an overlapping match of that offset
            if name.startswith("period{}@".format(p)):
                facts["overlapping match of offset {}".format(p)] = (s["pat_div"] if 64 % p == 0 else s["pat_nodiv"]) > 0
        for case, yes in facts.items():
            if yes:
                hit(case, name)
    return cov


def needed_cases():
    need = {("block", 0), ("block", 1), ("block", 2), ("lit", 0), ("lit", 1), ("lit", 2, 1), ("lit", 2, 4),
            ("lit", 3, 1), ("lit", 3, 4), ("weights", "fse"), ("weights", "direct"), "single", "window",
            "fcs0", "fcs1", "fcs2", "fcs4", "fcs8", ("seq", "none")}  # fmt: skip  (test_corpus_covers_every_mode)
    need |= {("seq", nm, m) for nm in ("LL", "OF", "ML") for m in range(4)}
    need |= {"block with more than kSeqBatch sequences", "Huffman stream longer than kLitWin",
             "Huffman literals, 1 stream", "Huffman literals, 4 streams", "Treeless literals in a later block",
             "more than one compressed block", "Raw block in a multi-block frame", "RLE block in a multi-block frame",
             "no content size", "output of 0 bytes", "output of 1 byte", "match with off >= ml",
             "match with off < ml, off divides 64", "match with off < ml, off does not divide 64", "off = 1",
             "barrier: source in the sequence's own literals",
             "barrier: source in the match before, not in own literals", "run of sequences without a barrier",
             "repeat offset"}  # fmt: skip
    need |= {"overlapping match of offset {}".format(p) for p in PERIODS}
    return need


def missing_cases(cov):
    return sorted(map(str, needed_cases() - set(cov)))


def coverage_report(cov):
    return "\n".join("{:<60} {:>4} frames, e.g. {}".format(str(c), len(cov[c]), cov[c][0])
                     for c in sorted(cov, key=str))  # fmt: skip


def blosc_level_frames():
    """(name, frame, raw): c-blosc's layouts of one image plane at every level of the corpus (2 MiB: two blocks of
    the largest size)."""
    plane = synth.synthetic_plane(5, 512, 2048).tobytes()
    return [("bs{} lv{}".format(bs, lv), zh.blosc_frame_cblosc_layout(plane, bs, lv), plane)
            for bs in (32 * 1024, 128 * 1024, 1 << 20) for lv in zh.LEVELS]  # fmt: skip


# ---- B: layouts ----------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 14, 15, 16, 17, 18, 30, 32, 34, 126, 128, 130, 510, 512, 514, 1022, 1024, 1026, 4094, 4096, 4098,
           1552, 70000, 70001)  # fmt: skip
ALIGNED_LENGTHS = (16, 128, 1024, 4096, 70000)  # once more with dst and src on 16 / 4 bytes: the wide paths


def _payload(n):
    """n bytes of image data followed by sparse and noisy stretches: literals and matches of every length."""
    base = _payload.cache
    if base is None:
        rng = np.random.default_rng(31)
        img = synth.synthetic_plane(8, 32, 1024).tobytes()  # 64 KiB
        sparse = np.zeros(4000, np.uint8)
        sparse[rng.integers(0, 4000, 60)] = 9
        base = _payload.cache = img[:50000] + sparse.tobytes() + rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    assert n <= len(base)
    return base[:n]


_payload.cache = None
_coded = {}


def _code(codec, part):
    key = (codec, part)
    if key not in _coded:
        _coded[key] = zh.zstd_compress(part, 3) if codec == eng_mod.TASK_ZSTD else baf.lz4_compress(part)
    return _coded[key]


def lz4_window_stream():
    """A hand-assembled LZ4 block longer than kLz4Win: short sequences up to just below the window's end, then a literal
    run that starts inside the first window and ends outside it, then sequences in the next window."""
    rng = np.random.default_rng(37)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    win = kernel_constants()["kLz4Win"]
    a = baf.Lz4Asm().lit(noise(32))
    while len(a.stream) + 40 < win - 60:
        a.match(int(rng.integers(1, 30)), int(rng.integers(4, 40))).lit(noise(int(rng.integers(1, 30))))
    a.match(5, 9).lit(noise(200))  # the run crosses the window's edge
    for _ in range(30):
        a.match(int(rng.integers(1, 300)), int(rng.integers(4, 90))).lit(noise(int(rng.integers(1, 14))))
    a.lit(noise(6 + (len(a.out) + len(a.pending)) % 2))
    return a.end()


def lz4_window_walk(stream):
    """The reads of ``lz_wave`` replayed next to ``baf.lz4_decompress_py``: the window is refilled at the first byte
    asked for outside it; a literal run is copied out of the window when it lies in it once its sequence is parsed,
    else out of the stream ("crossing": it began in a window and ran over its edge; "outside": any other).  Counts."""
    win = kernel_constants()["kLz4Win"]
    n = len(stream)
    state = {"lo": 0, "cnt": 0, "refills": 0}

    def at(p):
        if not state["lo"] <= p < state["lo"] + state["cnt"]:
            state["lo"], state["cnt"] = p, min(n - p, win)
            state["refills"] += 1
        return stream[p]

    def length(v, ip):
        if v == 15:
            while True:
                b = at(ip)
                ip += 1
                v += b
                if b != 255:
                    break
        return v, ip

    c = {"staged": 0, "crossing": 0, "outside": 0}
    ip = 0
    while True:
        token = at(ip)
        ll, ip = length(token >> 4, ip + 1)
        lit = ip
        ip += ll
        edge = state["lo"] + state["cnt"]  # of the window the run starts in (the token or its last length byte is there)
        if ip < n:
            at(ip), at(ip + 1)  # the offset: behind a run that leaves the window, this read moves the window past it
            _, ip = length(token & 15, ip + 2)
        lo, hi = state["lo"], state["lo"] + state["cnt"]
        if ll:
            if lit >= lo and lit + ll <= hi:  # (the test of lz_wave, after the whole sequence was parsed)
                c["staged"] += 1
            elif lit < edge < lit + ll:
                c["crossing"] += 1
            else:
                c["outside"] += 1
        if ip >= n:
            break
    c["refills"] = state["refills"]
    return c


def layout_table():
    """Section B: ``(table, facts)``; ``facts``: per task a dict of what decides the kernel's path."""
    E = eng_mod
    t, facts = Table(), []
    k = [0]

    def put(name, payload, n, kind, expect, aligned, fill=None, **fact):
        res = (0, 0) if aligned else (k[0] % 16, k[0] % 4)
        i = t.add(name, payload, n, kind, expect, dst_res=res[0], src_res=res[1], fill=fill)
        k[0] += 1
        r = t.rows[i]
        facts.append(dict(fact, kind=kind & 0xFF, flag=kind & (E.TASK_SHUFFLE | E.TASK_BITSHUFFLE),
                          split=bool(kind & E.TASK_SPLIT), n=n, dst=r[1], src=r[0]))  # fmt: skip

    def one_length(n, aligned):
        tag = "{}{}".format(n, " aligned" if aligned else "")
        raw = _payload(n)
        put("fill " + tag, b"", n, E.TASK_FILL, (struct.pack("<H", 0xA55A) * (n // 2 + 1))[:n], aligned, fill=0xA55A)
        for flag in FLAGS:
            st = stored_form(raw, flag)
            assert decoded_form(st, flag) == raw
            for kind, kn in ((E.TASK_COPY, "copy"), (E.TASK_STORED, "stored")):
                put("{} {:#x} {}".format(kn, flag, tag), st, n, kind | flag, raw, aligned)
            for codec, cn in ((E.TASK_ZSTD, "zstd"), (E.TASK_LZ4, "lz4")):
                z = _code(codec, st)
                put("{} {:#x} {}".format(cn, flag, tag), z, n, codec | flag, raw, aligned, stream=len(z))
                if n % 2:
                    continue
                ne = n // 2
                halves = (st[:ne], st[ne:])
                for coded in ((1, 1), (1, 0), (0, 1), (0, 0)):
                    parts = []
                    for h, c in zip(halves, coded):
                        z = _code(codec, h) if c else h
                        if c and len(z) == ne:  # a stream as long as its share would be read as stored: another coding
                            alts = ([zh.zstd_compress(h, lv) for lv in (-5, 19)] if codec == E.TASK_ZSTD
                                    else [baf.lz4_sequence(h)])  # fmt: skip
                            z = [a for a in alts if len(a) != ne][0]
                        assert (len(z) != ne) == bool(c), (tag, len(z))  # a coded stream is never as long as its share
                        parts.append(struct.pack("<I", len(z)) + z)
                    put("{} split{} {:#x} {}".format(cn, coded, flag, tag), b"".join(parts), n,
                        codec | flag | E.TASK_SPLIT, raw, aligned)  # fmt: skip

    for n in LENGTHS:
        one_length(n, False)
    for n in ALIGNED_LENGTHS:
        one_length(n, True)
    stream, raw = lz4_window_stream()
    put("lz4 hand-made stream over the window's edge", stream, len(raw), E.TASK_LZ4, raw, False, stream=len(stream),
        lz4_walk=lz4_window_walk(stream))  # fmt: skip
    return t, facts


def layout_paths(facts):
    """{path of the kernel: number of tasks that take it}, from the table alone.  The output and the scratch buffer
    are allocations (aligned far beyond 16 bytes), so a pointer's residue is its offset's."""
    E = eng_mod
    win = kernel_constants()["kLz4Win"]
    paths = {}

    def hit(name, yes=True):
        paths[name] = paths.get(name, 0) + (1 if yes else 0)

    for f in facts:
        n, kind = f["n"], f["kind"]
        if kind == E.TASK_FILL:
            continue
        plain = kind in (E.TASK_COPY, E.TASK_STORED)
        if f["flag"] == E.TASK_SHUFFLE:
            s_res = f["src"] if plain else f["dst"]  # a coded task un-shuffles out of scratch + dst
            wide = (f["dst"] | s_res | (n // 2)) & 3 == 0
            hit("wave_unshuffle aligned", wide and n >= 8)
            hit("wave_unshuffle bytewise", not wide and n >= 2)
            hit("wave_unshuffle bytewise, dst % 4 = {}".format(f["dst"] % 4), not wide and n >= 2)
            hit("wave_unshuffle odd tail", n % 2 == 1)
        elif f["flag"] == E.TASK_BITSHUFFLE:
            shuffled = n // 2 != 0 and (n // 2) % 8 == 0
            hit("wave_unbitshuffle, dst on 16 bytes", shuffled and f["dst"] % 16 == 0)
            hit("wave_unbitshuffle, dst not on 16 bytes", shuffled and f["dst"] % 16 != 0)
            hit("wave_unbitshuffle, elements not a multiple of 8 (copied)", not shuffled and n > 0)
        elif plain:
            hit("wave_copy with its 512-byte main loop", n >= 512)
            hit("wave_copy without its main loop", 0 < n < 512)
        if kind == E.TASK_LZ4 and not f["split"]:
            hit("LZ4 stream longer than kLz4Win", f["stream"] > win)
        if "lz4_walk" in f:
            w = f["lz4_walk"]
            hit("LZ4 window refilled", w["refills"] >= 2)
            hit("LZ4 literal run in the window", w["staged"] > 0)
            hit("LZ4 literal run over the window's edge", w["crossing"] > 0)
    for r in range(16):
        hit("dst % 16 = {}".format(r), any(f["dst"] % 16 == r for f in facts))
    for r in range(4):
        hit("src % 4 = {}".format(r), any(f["src"] % 4 == r and f["kind"] != E.TASK_FILL for f in facts))
    return paths


# ---- the status table --------------------------------------------------------------------------------------------------------
STATUS_TABLE = os.path.join(HERE, "golden", "zdec_task_statuses.npz")


def status_table(who):
    """The table of tools/make_golden_zdec_statuses.py -- every kind 0 .. 7 under the flag words 0, 0x100, 0x200, 0x400,
    0x300, 0x600, 0x500, 0x800 with a valid, a cut and a raw payload, 32 bytes of output each, and an odd split task per
    kind -- with the statuses and the bytes on record for ``who`` ("host": ``dsx_blosc_decode_ref``, "device": the
    kernels on an MI355X), both of the commit before the three host task runners became one."""
    rec = np.load(STATUS_TABLE)
    t = Table()
    t.packed = bytearray(rec["packed"].tobytes())
    t.rows = [tuple(int(v) for v in r) for r in rec["rows"]]
    t.names = [str(n) for n in rec["names"]]
    t.status = [int(s) for s in rec[who + "_status"]]
    t.expect = [rec[who + "_out"][i, : r[3]].tobytes() if st == 0 else None for i, (r, st) in enumerate(zip(t.rows, t.status))]
    t.end = max(r[1] + r[3] for r in t.rows)
    return t


# ---- C: malformed zstd tasks ---------------------------------------------------------------------------------------------
def malformed_cases():
    """[(name, task bytes, dst_len, kind, documented status or None)]: a fixed list."""
    E = eng_mod
    out = []
    for name, (frame, n, st) in zh._broken_frames().items():
        out.append((name, frame, n, E.TASK_ZSTD, st))
    for tag, (frame, data) in (("hand", zh._hand_frame()), ("hand fcs8", zh._hand_frame_fcs8())):
        for cut in range(len(frame)):
            out.append(("{} cut at {}".format(tag, cut), frame[:cut], len(data), E.TASK_ZSTD, E_TRUNCATED))
        out.append((tag + " with a byte appended", frame + b"\x00", len(data), E.TASK_ZSTD, E_TRUNCATED))
    hdr = struct.pack("<I", 0xFD2FB528) + bytes([0x20, 4])
    two = hdr + (0 | (0 << 1) | (4 << 3)).to_bytes(3, "little") + b"abcd" + b"\x01\x00"  # 2 of the 3 header bytes
    out.append(("second block header cut off", two, 4, E.TASK_ZSTD, E_TRUNCATED))
    data = periodic_data()["period7"][:600]
    good = zh.zstd_compress(data, 3)
    out.append(("wrong dst_len under TASK_SHUFFLE", good, len(data) + 2, E.TASK_ZSTD | E.TASK_SHUFFLE, E_OUTPUT))
    halves = [zh.zstd_compress(h, 3) for h in (data[:300], data[300:])]
    split = b"".join(struct.pack("<I", len(z)) + z for z in halves)
    out.append(("wrong dst_len under TASK_SPLIT", split, len(data) + 2, E.TASK_ZSTD | E.TASK_SPLIT, E_OUTPUT))
    out.append(("odd dst_len under TASK_SPLIT", split, len(data) + 1, E.TASK_ZSTD | E.TASK_SPLIT, E_OUTPUT))
    return out


E_TRUNCATED, E_OUTPUT = 1, 12  # csrc/dsx_zstd_dec.h Status


def good_neighbours(frames):
    """Small frames of section A to stand between the malformed tasks."""
    names = ("seven@1", "small_text@19", "period7@1", "period65@19", "hand", "one@3", "empty@5")
    good = [f for f in frames if f[0] in names]
    assert len(good) == len(names)
    return good


def malformed_table(good_frames):
    """Section C: every malformed case between good tasks (``good_frames``: small frames of section A), at the
    residues of section B."""
    t = Table()
    cases = malformed_cases()
    for i, (name, payload, n, kind, st) in enumerate(cases):
        g = good_frames[i % len(good_frames)]
        t.add("good " + g[0], g[1], len(g[2]), eng_mod.TASK_ZSTD, g[2], dst_res=(2 * i) % 16, src_res=(2 * i) % 4)
        t.add(name, payload, n, kind, None, status=st, dst_res=(2 * i + 1) % 16, src_res=(2 * i + 1) % 4)
    g = good_frames[0]
    t.add("good " + g[0], g[1], len(g[2]), eng_mod.TASK_ZSTD, g[2])
    return t
