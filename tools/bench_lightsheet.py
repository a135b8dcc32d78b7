"""Throughput of the light-sheet background mode (filtering.correct_lightsheet): device-resident uint16 planes in,
uint16 planes out, the defaults (percentile .25, artifact_length 150, background_window_size 200,
lightsheet_vs_background 2).  Prints one JSON line: the median of --steps timed runs, and with --host N the seconds
per plane of the host build (dsx_lightsheet_ref, one thread) over N planes and the ratio of the two rates.

    python tools/bench_lightsheet.py [--planes 64] [--steps 3] [--warmup 1] [--size 2048] [--max-batch 32] [--host 1]
                                     [--percentile P] [--artifact-length A] [--background-window-size B]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from aind_smartspim_destripe_amd import engine  # noqa: E402


def planes(count, S):
    """Background of ~200 counts with shot noise, an additive glow along x on a third of the rows, sparse bright cells."""
    rng = np.random.default_rng(0)
    block = rng.poisson(200.0, size=(count, S, S)).astype(np.float64)
    glow = rng.integers(0, 400, size=(count, S, 1)) * (rng.random((count, S, 1)) < 0.3)
    block += glow * (0.5 + 0.5 * np.cos(np.arange(S) / S * 3.0))[None, None, :]
    block[rng.random(block.shape) < 0.03] += 1500.0
    return np.clip(block, 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--host", type=int, default=0, help="planes to time through the host build (0: none)")
    ap.add_argument("--percentile", type=float, default=0.25)
    ap.add_argument("--artifact-length", type=int, default=150)
    ap.add_argument("--background-window-size", type=int, default=200)
    args = ap.parse_args()
    n, S = args.planes, args.size
    prm = dict(percentile=args.percentile, artifact_length=args.artifact_length,
               background_window_size=args.background_window_size, lightsheet_vs_background=2.0)  # fmt: skip
    block = planes(8, S)
    eng = engine.DestripeEngine(0)
    eng.plan_lightsheet(S, S, max_batch=args.max_batch, **prm)
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
    rate = n / statistics.median(times)
    result = {
        "metric": "light-sheet background mode: {0}x{0} uint16 planes/s, device-resident, p {1:g}, A {2}, B {3}, "
                  "uint16 out".format(S, args.percentile, args.artifact_length, args.background_window_size),
        "value": round(rate, 2),
        "unit": "planes/s",
        "planes": n,
        "max_batch": args.max_batch,
        "step_seconds": [round(t, 6) for t in times],
        "out_checksum": int(out.astype(np.uint64).sum()),
    }  # fmt: skip
    if args.host > 0:
        t0 = time.perf_counter()
        for k in range(args.host):
            ref = engine.lightsheet_ref(block[k % 8], out_dtype=np.uint16, **prm)[0]
        host_s = (time.perf_counter() - t0) / args.host
        result.update(host_seconds_per_plane=round(host_s, 4), host_planes_per_s=round(1.0 / host_s, 4),
                      device_over_host_thread=round(rate * host_s, 1), device_equals_host=bool(np.array_equal(ref, out[0]))
                      if args.host == 1 else None)  # fmt: skip
    print(json.dumps(result))
    d_in.free()
    d_out.free()
    eng.close()


if __name__ == "__main__":
    main()
