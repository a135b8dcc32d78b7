"""Writes tests/golden/zdec_task_statuses.npz (TEST INFRASTRUCTURE ONLY; not run by the suite).

    python tools/make_golden_zdec_statuses.py            the table and what dsx_blosc_decode_ref makes of it
    python tools/make_golden_zdec_statuses.py --device   adds what dsx_blosc_decode_device makes of it (needs a GPU)

One task table over the whole task model (``csrc/dsx_zdec_task.h``): every kind 0 .. 7 (7 is none) under the flag
words 0, 0x100, 0x200, 0x400, 0x300, 0x600, 0x500 and 0x800 (the last is no flag), each with three payloads -- a valid
stream of the kind for every share of the block, the same bytes without the last one, and ``dst_len`` raw bytes.  The
outputs are 32 bytes, two shares of 16: the smallest size at which the bit un-shuffle is active.  One task of 31 bytes
per kind asks for two streams of an odd length.  The streams come from the generators of the case tables
(``zdec_cases._code``, ``inflate_cases.code``).

The file records the table itself (the bytes of libzstd's frames may differ between its versions) and, per task, the
status and -- where it is 0 -- the output bytes of the library THIS SCRIPT RUNS WITH.  It is the record of the commit
before the three host task runners became one: run it there, not on a later commit whose answers it is to judge.
tests/test_zdec_task_statuses.py and tests/test_gpu_zdec_task_statuses.py hold the host runner and the kernels to it.
"""

import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "zdec_task_statuses.npz")
KINDS = range(8)
FLAG_WORDS = (0, 0x100, 0x200, 0x400, 0x300, 0x600, 0x500, 0x800)
N, SPLIT = 32, 0x200
FILL_VALUES = (0xA55A, 0x00A5, 0x1234)  # a fill task has no bytes: its three "payloads" are three values


def build_table():
    import inflate_cases as ic
    import zdec_cases as zc
    from aind_smartspim_destripe_amd import engine as E

    raw = (b"abcdabcdabcdabcX" + b"0123012301230123")[:N]  # (matches in either share, and across them)

    def stream(kind, part):
        if kind in (E.TASK_ZSTD, E.TASK_LZ4):
            z = zc._code(kind, part)
        elif kind in (E.TASK_ZLIB, E.TASK_BLOSCLZ):
            z = ic.code(kind, part)
            if len(z) == len(part):
                z = ic.code(kind, part, alt=True)
        else:
            return part  # copy, stored, and the kind that is none: the bytes themselves
        assert len(z) != len(part), (kind, len(z))  # (as long as its share, a stream of a split task is stored)
        return z

    def valid(kind, word, n):
        if not word & SPLIT:
            return stream(kind, raw[:n])
        ne = n // 2
        parts = [stream(kind, h) for h in (raw[:ne], raw[ne : 2 * ne])]
        return b"".join(struct.pack("<I", len(z)) + z for z in parts)

    t = zc.Table()
    for kind in KINDS:
        for word in FLAG_WORDS:
            good = valid(kind, word, N)
            payloads = (("valid", good), ("cut", good[:-1]), ("raw", raw))
            for j, (pn, payload) in enumerate(payloads):
                fill = FILL_VALUES[j] if kind == E.TASK_FILL else None
                t.add("kind {} flags {:#x} {}".format(kind, word, pn), payload, N, kind | word, None, status=None, fill=fill)
        fill = FILL_VALUES[0] if kind == E.TASK_FILL else None
        t.add("kind {} flags {:#x} valid, 31 bytes".format(kind, SPLIT), valid(kind, SPLIT, N), N - 1, kind | SPLIT, None,
              status=None, fill=fill)  # fmt: skip
    return t


def record(table, out, status):
    """(statuses, [tasks, N] output bytes: those of the tasks with status 0, zeros elsewhere)"""
    got = np.zeros((len(table.rows), N), np.uint8)
    for i, r in enumerate(table.rows):
        if status[i] == 0:
            got[i, : r[3]] = out[r[1] : r[1] + r[3]]
    return status.astype(np.int32), got


def main():
    import zdec_cases as zc
    from aind_smartspim_destripe_amd import engine as E

    t = build_table()
    out = {"packed": np.frombuffer(bytes(t.packed), np.uint8), "rows": np.array(t.rows, np.int64),
           "names": np.array(t.names)}  # fmt: skip
    out["host_status"], out["host_out"] = record(t, *zc.run_ref(t))
    if "--device" in sys.argv[1:]:
        e = E.DestripeEngine(0)
        try:
            out["device_status"], out["device_out"] = record(t, *zc.run_device(e, t))
        finally:
            e.close()
        differ = np.flatnonzero((out["host_status"] != out["device_status"]) | (out["host_out"] != out["device_out"]).any(1))
        print("tasks on which the host and the device disagree:", [t.names[i] for i in differ] or "none")
    elif os.path.exists(OUT):  # keep the device's record of the same table
        old = np.load(OUT)
        if "device_status" in old and np.array_equal(old["rows"], out["rows"]) and np.array_equal(old["packed"], out["packed"]):
            out["device_status"], out["device_out"] = old["device_status"], old["device_out"]
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else OUT
    np.savez_compressed(dest, **out)
    st = out["host_status"]
    print(len(t.rows), "tasks,", len(t.packed), "packed bytes; host statuses:",
          {int(s): int((st == s).sum()) for s in np.unique(st)}, "->", dest, os.path.getsize(dest), "bytes")


if __name__ == "__main__":
    main()
