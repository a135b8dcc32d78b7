#!/usr/bin/env python3
"""Dispatches of k_volhist_u16 on one 64 x 2048 x 2048 uint16 block (537 MB) per kind of data, next to
k_planes_to_bricks of the same block, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/volhist_cases.py [reps]

Every case is checked against np.bincount first (the result must be exact whatever the contention), then dispatched
`reps` times (default 10) after one warm-up; the cases run in the order of CASES, so the k-th group of `reps + 2`
k_volhist_u16 rows of the trace (check, warm-up, reps) is the k-th case.  Prints one JSON line with the order, and the
per-case time from device events around the `reps` dispatches (a cross-check of the trace, not a replacement)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import engine as eng_mod, synth

Z, H, W = 64, 2048, 2048
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rs = np.random.RandomState(7)


def background():  # what a destriped plane without tissue looks like: a level with a few counts of noise
    return (150 + rs.poisson(9.0, (Z, H, W)) - 9).astype(np.uint16)


CASES = [
    ("constant 150 (one LDS bin, worst contention inside the window)", lambda: np.full((Z, H, W), 150, np.uint16)),
    ("constant 40000 (one global bin, outside the window)", lambda: np.full((Z, H, W), 40000, np.uint16)),
    ("background 150 +- 3 (Poisson noise)", background),
    ("synthetic stack (synth.synthetic_stack: tissue, cells, stripes)", lambda: synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(8, H, W))),
    ("uniform random 0 .. 65535 (3/4 of the voxels outside the window)", lambda: rs.randint(0, 65536, (Z, H, W)).astype(np.uint16)),
]

eng = eng_mod.DestripeEngine(0)
d_vol, d_bricks = eng.alloc(Z * H * W * 2), eng.alloc(Z * H * W * 2)
out = {"block": [Z, H, W], "reps": reps, "cases": []}
try:
    for name, make in CASES:
        vol = make()
        d_vol.upload(vol)
        eng.volhist_reset()
        eng.volhist_add(d_vol, vol.size)
        exact = bool(np.array_equal(eng.volhist_get(), np.bincount(vol.ravel(), minlength=65536)))
        eng.volhist_add(d_vol, vol.size)  # warm-up
        eng.sync()
        eng.timer_start()
        for _ in range(reps):
            eng.volhist_add(d_vol, vol.size)
        ms = eng.timer_stop() / reps
        out["cases"].append({"case": name, "exact": exact, "event_ms_per_dispatch": round(ms, 4),
                             "read_TBps": round(vol.nbytes / ms / 1e9, 2), "values_present": int(np.unique(vol[0]).size)})
        if not exact:
            break
    eng.planes_to_bricks(d_vol, d_bricks, (Z, H, W), (64, 128, 128))  # the yardstick: reads and writes the block once
    eng.sync()
    eng.timer_start()
    for _ in range(reps):
        eng.planes_to_bricks(d_vol, d_bricks, (Z, H, W), (64, 128, 128))
    out["planes_to_bricks_event_ms"] = round(eng.timer_stop() / reps, 4)
finally:
    d_vol.free()
    d_bricks.free()
    eng.close()
print(json.dumps(out))
sys.exit(0 if all(c["exact"] for c in out["cases"]) else 3)
