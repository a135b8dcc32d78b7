"""Writes tests/golden/encoder_frames.json (TEST INFRASTRUCTURE ONLY; not run by the suite).

    python tools/make_golden_encoder_frames.py [--out FILE]

For every case of tests/encoder_golden_cases.py, every mode of the Blosc encoders and the mode's level and level 0: the
sha256 of the packed frames and of the offsets that ``engine.blosc_encode_ref`` (the host build, which the kernels must
match byte for byte) produces, and the frames' total bytes.  Digests only: a few KB.

The file is the record of the commit it names -- the one before the encoders came to share one frame writer.  To
record, copy this script and tests/encoder_golden_cases.py into a built checkout of THAT commit (a ``git worktree``,
say) and run it there, not on a later commit whose bytes it is to judge; then copy the file here.
tests/test_encoder_golden.py and tests/test_gpu_encoder_golden.py hold the host builds and the kernels to it.
"""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import encoder_golden_cases as gc
    from aind_smartspim_destripe_amd import engine as E

    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    digests = {}
    for name, chunks in gc.cases():
        for mode, clevel in gc.settings():
            digests[gc.key(name, mode, clevel)] = gc.digest(*E.blosc_encode_ref(chunks, clevel, mode=mode))
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else gc.GOLDEN
    with open(dest, "w") as f:
        json.dump({"commit": commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(digests), "encodings of", len(gc.cases()), "cases at", commit[:7], "->", dest, os.path.getsize(dest), "bytes")


if __name__ == "__main__":
    main()
