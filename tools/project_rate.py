#!/usr/bin/env python3
"""Dispatches of k_project_u16 / k_project_fold on one 64-plane uint16 block, next to k_volhist_u16 of the same block
(it also reads the block once), for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/project_rate.py [reps] [H W]

The block is synth.synthetic_stack (tissue, cells, stripes), 64 x 2048 x 2048 (537 MB) by default.  The projections are
checked against NumPy first (exact), then each kernel is dispatched `reps` times (default 10) after one warm-up, the
projections with first=False as every block of a pass but the first runs.  Prints one JSON line with the time per
dispatch from device events around the `reps` dispatches (a cross-check of the trace, not a replacement)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import engine as eng_mod, projections as pr, synth

Z = 64
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (2048, 2048)
vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(8, H, W))
want = pr.project_volume(vol)

eng = eng_mod.DestripeEngine(0)
d_vol = eng.alloc(vol.nbytes)
work_bytes = eng_mod.project_work_bytes(vol.shape)
d_work = eng.alloc(work_bytes)
bufs = eng.alloc_projection(vol.shape)
out = {"block": [Z, H, W], "reps": reps, "block_bytes": vol.nbytes, "work_bytes": work_bytes}
try:
    d_vol.upload(vol)
    eng.project(d_vol, vol.shape, bufs, d_work=d_work)
    got = eng.projection_get(bufs, vol.shape)
    out["exact"] = bool(all(np.array_equal(got[k], want[k]) for k in want))
    for name, run in (("project", lambda: eng.project(d_vol, vol.shape, bufs, first=False, d_work=d_work)),
                      ("volhist", lambda: eng.volhist_add(d_vol, vol.size))):
        if name == "volhist":
            eng.volhist_reset()
        run()  # warm-up
        eng.sync()
        eng.timer_start()
        for _ in range(reps):
            run()
        ms = eng.timer_stop() / reps
        out[name] = {"event_ms_per_dispatch": round(ms, 4), "read_TBps": round(vol.nbytes / ms / 1e9, 2)}
finally:
    for b in [d_vol, d_work] + list(bufs.values()):
        b.free()
    eng.close()
print(json.dumps(out))
sys.exit(0 if out.get("exact") else 3)
