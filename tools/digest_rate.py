#!/usr/bin/env python3
"""Dispatches of k_brick_digest_u16 on one 64-plane uint16 block in (64, 128, 128) bricks, next to k_volhist_u16 over the
same bytes (it also reads them once), for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/digest_rate.py [reps] [H W]

The block is synth.synthetic_stack (tissue, cells, stripes), 64 x 2048 x 2048 (537 MB) by default, re-tiled on the device
(planes_to_bricks) as the store pass leaves it.  The records are checked against the host build first (exact), then each
kernel is dispatched `reps` times (default 10) after one warm-up.  Prints one JSON line with the time per dispatch from
device events around the `reps` dispatches (a cross-check of the trace, not a replacement)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import engine as eng_mod, synth

Z, C = 64, (64, 128, 128)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (2048, 2048)
vol = synth.synthetic_stack(Z, H, W, bank=synth.synthetic_bank(8, H, W))
grid = (1, -(-H // C[1]), -(-W // C[2]))
n = grid[1] * grid[2]
brick = int(np.prod(C))

eng = eng_mod.DestripeEngine(0)
d_vol, d_bricks, d_rec = eng.alloc(vol.nbytes), eng.alloc(n * brick * 2), eng.alloc(n * eng_mod.DIGEST_DTYPE.itemsize)
out = {"block": [Z, H, W], "bricks": list(grid), "chunks": list(C), "reps": reps, "block_bytes": n * brick * 2}
try:
    d_vol.upload(vol)
    eng.planes_to_bricks(d_vol, d_bricks, (Z, H, W), C, 0)
    eng.brick_digest(d_bricks, grid, C, (Z, H, W), d_rec)
    eng.sync()
    got = d_rec.download((n,), eng_mod.DIGEST_DTYPE)
    want = eng_mod.brick_digest_ref(d_bricks.download((n * brick,), np.uint16), grid, C, (Z, H, W))
    out["exact"] = bool(np.array_equal(got, want)) and int(got["count"].sum()) == Z * H * W
    for name, run in (("digest", lambda: eng.brick_digest(d_bricks, grid, C, (Z, H, W), d_rec)),
                      ("volhist", lambda: eng.volhist_add(d_bricks, n * brick))):
        if name == "volhist":
            eng.volhist_reset()
        run()  # warm-up
        eng.sync()
        eng.timer_start()
        for _ in range(reps):
            run()
        ms = eng.timer_stop() / reps
        out[name] = {"event_ms_per_dispatch": round(ms, 4), "read_TBps": round(n * brick * 2 / ms / 1e9, 2)}
finally:
    for b in (d_vol, d_bricks, d_rec):
        b.free()
    eng.close()
print(json.dumps(out))
sys.exit(0 if out.get("exact") else 3)
