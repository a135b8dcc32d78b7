"""Rate of the stack-rank kernel (DestripeEngine.stack_rank, csrc/dsx_stackrank.h) on a device-resident stack of
--planes x --height x --width uint16 synthetic planes, for the quantile sets (500) and (500, 50): --runs interleaved
runs per arm, each the median of --steps timed launches.  The yardstick is the host build (dsx_stack_rank_u16_ref) on
one thread over the first 1 / --host-share of every plane's pixels, scaled up by that share; its output must equal the
device's on those pixels.  Prints one JSON line; --out writes the same record, indented.

    python tools/bench_flat_estimation.py [--planes 256] [--height 1600] [--width 2000] [--runs 3] [--steps 3]
                                          [--warmup 1] [--host-share 16] [--out profiles/flat_estimation_bench.json]

--trace N: no timing; N launches of each arm and N of k_volhist_u16 over the same buffer, for a run under
rocprofv3 --kernel-trace --stats (a run of its own).
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from aind_smartspim_destripe_amd import engine, synth  # noqa: E402

ARMS = {"q500": (500,), "q500_q50": (500, 50)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=256)
    ap.add_argument("--height", type=int, default=1600)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-share", type=int, default=16, help="the host build ranks 1 / this of the pixels (0: no host run)")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.planes, args.height, args.width
    P = H * W
    bank = synth.synthetic_bank(min(32, n), H, W)
    eng = engine.DestripeEngine(0)
    d_stack = eng.alloc(2 * n * P)
    for z in range(n):  # synth.synthetic_stack, plane by plane
        d_stack.upload(np.roll(bank[z % len(bank)], z // len(bank), axis=0), offset=2 * z * P)
    d_out, d_valid = eng.alloc(2 * 2 * P), eng.alloc(2 * P)

    if args.trace:
        eng.volhist_reset()
        for _ in range(args.trace):
            eng.volhist_add(d_stack, n * P)
            for q in ARMS.values():
                eng.stack_rank(d_stack, n, P, q, d_out=d_out, d_valid=d_valid)
        eng.sync()
        print(json.dumps({"trace": args.trace, "stack_bytes": 2 * n * P, "arms": {k: list(v) for k, v in ARMS.items()}}))
        return

    for q in ARMS.values():
        for _ in range(args.warmup):
            eng.stack_rank(d_stack, n, P, q, d_out=d_out, d_valid=d_valid)
    eng.sync()
    runs = {name: [] for name in ARMS}
    for _ in range(args.runs):
        for name, q in ARMS.items():  # interleaved
            times = []
            for _ in range(args.steps):
                eng.timer_start()
                eng.stack_rank(d_stack, n, P, q, d_out=d_out, d_valid=d_valid)
                times.append(eng.timer_stop() / 1e3)
            runs[name].append({"seconds": round(statistics.median(times), 6), "step_seconds": [round(t, 6) for t in times]})
    eng.sync()
    result = {"tool": "tools/bench_flat_estimation.py",
              "workload": "{} x {} x {} uint16 planes of synth, device-resident, full window".format(n, H, W),
              "stack_bytes": 2 * n * P, "arms": {}}  # fmt: skip
    for name, q in ARMS.items():
        med = statistics.median(r["seconds"] for r in runs[name])
        result["arms"][name] = {"q_milli": list(q), "runs": runs[name], "median_seconds": round(med, 6),
                                "stack_TB_per_s": round(2 * n * P / med / 1e12, 3)}  # fmt: skip

    if args.host_share > 0:
        share = P // args.host_share
        part = np.empty((n, share), np.uint16)
        for z in range(n):
            part[z] = np.roll(bank[z % len(bank)], z // len(bank), axis=0).reshape(-1)[:share]
        host = {"what": "dsx_stack_rank_u16_ref on one thread of the same machine over the first 1/{} of every plane's "
                        "pixels ({} of {}), seconds scaled by {}".format(args.host_share, share, P, args.host_share)}  # fmt: skip
        for name, q in ARMS.items():
            eng.stack_rank(d_stack, n, P, q, d_out=d_out, d_valid=d_valid)
            eng.sync()
            dev = d_out.download((len(q), P), np.uint16)[:, :share]
            dev_valid = d_valid.download((P,), np.uint16)[:share]
            t0 = time.perf_counter()
            ref, ref_valid = engine.stack_rank_ref(part, q)
            seconds = (time.perf_counter() - t0) * P / share
            equal = bool(np.array_equal(ref, dev) and np.array_equal(ref_valid, dev_valid))
            host[name] = {"scaled_seconds": round(seconds, 3), "output_equals_device": equal,
                          "device_over_one_host_thread": round(seconds / result["arms"][name]["median_seconds"], 1)}  # fmt: skip
        result["host_build"] = host
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    for d in (d_stack, d_out, d_valid):
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
