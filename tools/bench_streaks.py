"""Throughput of the dual-band wavelet-FFT filter (filter_streaks with sigma = (fg, bg)): device-resident uint16
planes in, uint16 planes out, db3, maximum level, Otsu per plane.  Prints one JSON line; frac uses bench.py's
16 777 216 bytes per 2048 x 2048 plane (uint16 in + uint16 out, read and written once) against 8 TB/s.

    python tools/bench_streaks.py [--planes 256] [--steps 5] [--warmup 2] [--size 2048] [--max-batch 32]
                                  [--route generic|march|auto] [--bands both|fg|bg] [--smoothing S] [--shading]

--bands / --smoothing / --shading time the options of the blend (README "filter_streaks"): one filtered band, the
gaussian over the blend weight, and a dark / flat step (a flat in [0.8, 1.2], a dark of 100).
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from aind_smartspim_destripe_amd import engine  # noqa: E402

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--sigma", type=float, nargs=2, default=(64.0, 128.0))
    ap.add_argument("--crossover", type=float, default=10.0)
    ap.add_argument("--route", default="generic", choices=("generic", "march", "auto"))
    ap.add_argument("--bands", default="both", choices=("both", "fg", "bg"))
    ap.add_argument("--smoothing", type=float, default=0.0)
    ap.add_argument("--shading", action="store_true")
    args = ap.parse_args()
    n, S = args.planes, args.size
    rng = np.random.default_rng(0)
    block = rng.poisson(200.0, size=(8, S, S)).astype(np.float64)
    block += 60.0 * np.sin(np.arange(S) / 5.0)[None, :, None]
    block[rng.random(block.shape) < 0.03] += 1500.0
    block = np.clip(block, 0, 65535).astype(np.uint16)
    eng = engine.DestripeEngine(0)
    flat = (0.8 + 0.4 * rng.random((S, S))).astype(np.float32) if args.shading else None
    dark = np.full((S, S), 100.0, np.float32) if args.shading else None
    eng.plan_streaks(S, S, args.sigma[0], args.sigma[1], wavelet="db3", level=0, crossover=args.crossover,
                     threshold=None, max_batch=args.max_batch, route=args.route, bands=args.bands,
                     smoothing=args.smoothing, flatfield=flat, darkfield=dark)  # fmt: skip
    plane_bytes = S * S * 2
    d_in = eng.alloc(plane_bytes * n)
    d_out = eng.alloc(plane_bytes * n)
    for k in range(0, n, 8):
        m = min(8, n - k)
        d_in.upload(block[:m], offset=k * plane_bytes)
    for _ in range(args.warmup):
        eng.run_device(d_in, np.uint16, n, d_out, np.uint16)
    eng.sync()
    times = []
    for _ in range(args.steps):
        eng.timer_start()
        eng.run_device(d_in, np.uint16, n, d_out, np.uint16)
        times.append(eng.timer_stop() / 1e3)
    eng.sync()
    out = d_out.download((1, S, S), np.uint16)
    best = min(times)
    rate = n / best
    achieved = rate * 16777216 * (S * S) / (2048 * 2048) / 1e9
    print(json.dumps({
        "metric": "dual-band streaks filter: {0}x{0} uint16 planes/s, device-resident, db3, sigma=({1:g}, {2:g}), "
                  "crossover {3:g}, max level, Otsu per plane, uint16 out".format(S, args.sigma[0], args.sigma[1],
                                                                                 args.crossover),
        "value": round(rate, 2),
        "unit": "planes/s",
        "route": eng.streaks_route,
        "bands": args.bands,
        "smoothing": args.smoothing,
        "shading": bool(args.shading),
        "planes": n,
        "max_batch": args.max_batch,
        "step_seconds": [round(t, 6) for t in times],
        "achieved_GBs": round(achieved, 2),
        "frac": round(achieved / HBM_PEAK_GBS, 5),
        "out_checksum": int(out.astype(np.uint64).sum()),
    }))  # fmt: skip
    d_in.free()
    d_out.free()
    eng.close()


if __name__ == "__main__":
    main()
