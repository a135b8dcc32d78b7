#!/usr/bin/env python3
"""The pyramid kernels of one 64-plane block of 2048 x 2048 uint16 under a kernel trace: `k_pyramid_block` (levels 1 and
2 of the 2 x 2 x 2 pyramid in one read) next to the level steps of another scale, `k_pyramid_step<FZ, FY, FX>`.

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/pyramid_scale_rate.py [reps] [FZ-FY-FX]

Every repetition runs both scales with three levels (n_levels = 3: two written) into chunk rows (64, 128, 128), the
outputs zeroed once beforehand.  The line printed gives the bytes each kernel moves, so that bytes / traced duration is
its rate: k_pyramid_block reads level 0 (Z H W 2 bytes) and writes levels 1 and 2; the level-1 step reads level 0 and
writes level 1 twice (bricks and the dense copy for level 2)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import engine as eng_mod, pyramid

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
scale = tuple(int(f) for f in sys.argv[2].split("-")) if len(sys.argv) > 2 else (1, 2, 2)
zyx = (64, 2048, 2048)
e = eng_mod.DestripeEngine(0)
bufs = []
try:
    d_vol = e.alloc(int(np.prod(zyx)) * 2)
    bufs.append(d_vol)
    d_vol.upload(np.random.RandomState(0).randint(0, 65536, zyx).astype(np.uint16))
    plans = []
    for sc in ((2, 2, 2), scale):
        chunks = [lv.chunks for lv in pyramid.fused_levels((4096,) + zyx[1:], (64, 128, 128), 3, sc)]
        d_bricks = [e.alloc(eng_mod.pyramid_level_elems(zyx, l, c, 1, sc) * 2) for l, c in enumerate(chunks, start=1)]
        work = eng_mod.pyramid_work_bytes(zyx, 3, sc)
        d_work = e.alloc(work) if work else None
        bufs += d_bricks + ([d_work] if work else [])
        e.pyramid_block(d_vol, zyx, chunks, d_bricks, d_work=d_work, scale=sc)  # (zeroes the rows once)
        plans.append((sc, chunks, d_bricks, d_work))
    e.sync()
    for _ in range(reps):
        for sc, chunks, d_bricks, d_work in plans:
            e.pyramid_block(d_vol, zyx, chunks, d_bricks, zero=[False] * len(chunks), d_work=d_work, scale=sc)
    e.sync()
    level = lambda l, sc: int(np.prod([n // f**l for n, f in zip(zyx, sc)])) * 2  # noqa: E731
    print(json.dumps({"block": list(zyx), "reps": reps, "scale": list(scale),
                      "k_pyramid_block_bytes": {"read": level(0, (2, 2, 2)), "written": level(1, (2, 2, 2)) + level(2, (2, 2, 2))},
                      "level1_step_bytes": {"read": level(0, scale), "written": 2 * level(1, scale)},
                      "level2_step_bytes": {"read": level(1, scale), "written": level(2, scale)}}))
finally:
    for b in bufs:
        b.free()
    e.close()
