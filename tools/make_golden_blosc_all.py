"""Writes tests/golden/blosc_all_frames.npz with the real c-blosc (TEST INFRASTRUCTURE ONLY; not run by the suite).

    python tools/make_golden_blosc_all.py

The frames ``DSX_ZDEC_ALL`` adds to the device's share (``csrc/dsx_inflate.h``), made by c-blosc 1.21.0 itself
(``libblosc.so.1.21.0``, loaded with ctypes as oracle/make_golden_blosc.py does): blosclz and zlib inside, typesize 2,
all nine levels, no / byte / bit shuffle, payloads of 32 768 and 65 536 bytes (``brick``, ``runs``, ``noise`` of
tests/test_blosc.py::payload) with forced block sizes of 8 192 and 32 768 bytes.  This build of the library does not
go below blocks of 64 KiB whatever size is forced (the headers of the frames say so), so these frames have one block
each; four more frames of 140 000 bytes have two full blocks and a short last one.  The full cross product would be 20 MB; every (codec, level, shuffle) gets one
(payload, size, block size) combination, rotated so that every combination meets every codec and shuffle.
"""

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "blosc_all_frames.npz")
LIB = "/opt/conda/lib/libblosc.so.1.21.0"
COMBOS = (("brick", 65536, 32768), ("runs", 65536, 8192), ("brick", 32768, 8192), ("runs", 32768, 32768),
          ("noise", 32768, 8192), ("runs", 65536, 32768), ("brick", 32768, 32768), ("runs", 32768, 8192),
          ("brick", 65536, 8192))  # fmt: skip
LEFTOVER = ("runs", 140000, 8192)


def main():
    from test_blosc import payload

    lib = ctypes.CDLL(LIB)
    lib.blosc_get_version_string.restype = ctypes.c_char_p
    lib.blosc_compress_ctx.restype = ctypes.c_int
    lib.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.blosc_decompress_ctx.restype = ctypes.c_int
    lib.blosc_decompress_ctx.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    version = lib.blosc_get_version_string().decode()
    out = {"blosc_version": np.array(version)}
    total = i = 0
    # c-blosc 1.21 splits every full block of 2-byte elements, whatever the codec; only a short last block is one
    # stream: LEFTOVER adds four frames that have one behind two full blocks
    grid = [(ci, cname, clevel, shuffle, COMBOS[(clevel + 3 * shuffle + ci) % len(COMBOS)])
            for ci, cname in enumerate(("blosclz", "zlib")) for clevel in range(1, 10) for shuffle in (0, 1, 2)]  # fmt: skip
    grid += [(ci, cname, 5, shuffle, LEFTOVER) for ci, cname in enumerate(("blosclz", "zlib")) for shuffle in (1, 2)]
    for ci, cname, clevel, shuffle, (kind, nbytes, blocksize) in grid:
        seed = 100 + i
        if kind == "brick" and shuffle == 0:
            nbytes = 32768  # (unshuffled 16-bit samples barely compress: 65 536 bytes of them add size, not cases)
        while True:
            raw = payload(kind, seed, nbytes)
            cap = len(raw) + 16
            buf = ctypes.create_string_buffer(cap)
            n = lib.blosc_compress_ctx(clevel, shuffle, 2, len(raw), raw, buf, cap, cname.encode(), blocksize, 1)
            assert n > 0, (cname, clevel, shuffle, n)
            frame = buf.raw[:n]
            if not frame[2] & 0x2 or kind == "noise":
                break
            kind = "runs"  # c-blosc stored the frame whole (memcpyed), as it does noise: a payload it codes instead
        back = ctypes.create_string_buffer(len(raw))
        assert lib.blosc_decompress_ctx(frame, back, len(raw), 1) == len(raw) and back.raw[: len(raw)] == raw
        out["frame_%03d" % i] = np.frombuffer(frame, np.uint8)
        out["case_%03d" % i] = np.array("%s %d %d 2 %s %d %d %d" % (cname, clevel, shuffle, kind, seed, nbytes, blocksize))
        print(i, cname, clevel, shuffle, kind, nbytes, blocksize, "->", n, "bytes, flags 0x%02x" % frame[2])
        total += n
        i += 1
    np.savez_compressed(OUT, **out)  # (the stored frames of compressible payloads shrink; a committed file stays under 1 MiB)
    print("c-blosc", version, ":", i, "frames,", total, "bytes ->", OUT, os.path.getsize(OUT), "bytes on disk")


if __name__ == "__main__":
    main()
