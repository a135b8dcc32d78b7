"""Rate of the stack-rank kernel (DestripeEngine.stack_rank, csrc/dsx_stackrank.h) on a device-resident stack of
--planes x --height x --width uint16 synthetic planes, for the quantile sets (500) and (500, 50): --runs interleaved
runs per arm, each the median of --steps timed launches.  The yardstick is the host build (dsx_stack_rank_u16_ref) on
one thread over the first 1 / --host-share of every plane's pixels, scaled up by that share; its output must equal the
device's on those pixels.  Prints one JSON line; --out writes the same record, indented.

    python tools/bench_flat_estimation.py [--planes 256] [--height 1600] [--width 2000] [--runs 3] [--steps 3]
                                          [--warmup 1] [--host-share 16] [--out profiles/flat_estimation_bench.json]

--trace N: no timing; N launches of each arm and N of k_volhist_u16 over the same buffer, for a run under
rocprofv3 --kernel-trace --stats (a run of its own).

--finish: the finish of the flat instead (DestripeEngine.flat_finish, csrc/dsx_smooth.h) on the rank planes of the same
stack at --sigma, without and with a dark quantile: --runs interleaved runs per arm of the device finish (wall clock of the
call, which returns after the chain has run), of its host build on one thread (engine.flat_finish_ref) and of today's
NumPy finish (steps 2 to 4 of estimate_fields); the device must equal the host build bit for bit.  Then a whole
estimate_channel_flats under finish="numpy" and finish="native" over a synthetic channel of --channel-tiles tiles of
--channel-planes planes of the same plane size, with its LAST_ESTIMATE.  With --trace N: N launches of the rank kernel
(500, 50) and N finishes with a dark plane, for the kernel trace.

    python tools/bench_flat_estimation.py --finish [--sigma 32] [--runs 3] [--out profiles/flat_finish_bench.json]
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
from aind_smartspim_destripe_amd import flatfield_estimation as fe  # noqa: E402

ARMS = {"q500": (500,), "q500_q50": (500, 50)}


def numpy_finish(R, valid, sigma, floor):
    """Steps 2 to 4 of estimate_fields as it runs them under finish="numpy"."""
    seen = valid > 0
    planes = []
    for r in R:
        r = r.astype(np.float64)
        if not seen.all():
            r[~seen] = np.median(r[seen])
        planes.append(fe.gaussian_smooth(r, sigma))
    flat = np.maximum(planes[0] / planes[0].mean(), floor).astype(np.float32)
    return flat, (planes[1].astype(np.float32) if len(planes) > 1 else None)


def channel_arm(args, tmp):
    """estimate_channel_flats under both routes over a synthetic channel written to ``tmp``: LAST_ESTIMATE of each."""
    from aind_smartspim_destripe_amd import mini_tiff
    from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

    H, W, Z = args.height, args.width, args.channel_planes
    names = ["{}_{}".format(431040 + 26040 * t, 368180) for t in range(args.channel_tiles)]
    bank = synth.synthetic_bank(min(8, Z), H, W)
    for t, name in enumerate(names):
        a = MiniZarrArray.create(os.path.join(tmp, "data", "ch", name + ".zarr", "0"), (1, 1, Z, H, W), (1, 1, Z, 400, 400),
                                 np.uint16, compressor=None)  # fmt: skip
        a[0, 0] = np.stack([np.roll(bank[z % len(bank)], 7 * t + z // len(bank), axis=0) for z in range(Z)])
    params = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
    sides = {"0": names[: max(1, len(names) // 2)], "1": names[max(1, len(names) // 2) :]}
    sides = {k: v for k, v in sides.items() if v}
    out = {"what": "estimate_channel_flats over {} tiles of {} planes {} x {}, plane_step 1, sigma {}, dark_quantile 0.05, "
                   "{} laser side(s); seconds summed over the sides".format(len(names), Z, H, W, args.sigma, len(sides)), "runs": []}  # fmt: skip
    flats = {}
    for run in range(args.runs):
        rec = {}
        for route in fe.FINISH_ROUTES:  # interleaved
            paths = fe.estimate_channel_flats(os.path.join(tmp, "data"), "ch", sides, params, os.path.join(tmp, "flats_" + route),
                                              plane_step=1, smoothing=args.sigma, dark_quantile=0.05, finish=route)  # fmt: skip
            last = fe.LAST_ESTIMATE
            rec[route] = {"seconds": {k: round(v, 6) for k, v in last["seconds"].items()},
                          "finish": {"route": last["finish"]["route"],
                                     "seconds": {k: round(v, 6) for k, v in last["finish"]["seconds"].items()}}}  # fmt: skip
            flats[route] = [mini_tiff.imread(p) for p in paths]
        out["runs"].append(rec)
    out["median_estimate_seconds"] = {route: round(statistics.median(r[route]["seconds"]["estimate"] for r in out["runs"]), 6)
                                      for route in fe.FINISH_ROUTES}  # fmt: skip
    out["median_finish_seconds"] = {route: round(statistics.median(r[route]["finish"]["seconds"]["finish"] for r in out["runs"]), 6)
                                    for route in fe.FINISH_ROUTES}  # fmt: skip
    a, b = np.stack(flats["numpy"]), np.stack(flats["native"])
    out["native_within_one_float32_spacing_of_numpy"] = bool(np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(a, b))))
    out["flats_that_differ"] = int((a != b).sum())
    return out


def finish_bench(args, eng, d_stack, n, H, W):
    import tempfile

    P = H * W
    q = ARMS["q500_q50"]
    d_rank, d_valid = eng.stack_rank(d_stack, n, P, q)
    d_flat, d_dark = eng.alloc(4 * P), eng.alloc(4 * P)
    d_work = eng.alloc(engine.flat_finish_work_bytes((H, W)))
    r, taps = engine.gauss_taps(args.sigma)
    floor = 0.1
    arms = {"flat": 1, "flat_dark": 2}

    def device(n_q):
        eng.flat_finish(d_rank, d_valid, (H, W), (H, W), n_q, taps, floor, d_flat=d_flat, d_dark=d_dark, d_work=d_work)

    if args.trace:
        for _ in range(args.trace):
            eng.stack_rank(d_stack, n, P, q, d_out=d_rank, d_valid=d_valid)
            device(2)
        eng.sync()
        print(json.dumps({"trace": args.trace, "finish": True, "sigma": args.sigma, "radius": r, "shape": [H, W], "planes": n}))
        return
    eng.sync()
    R, valid = d_rank.download((2, H, W), np.uint16), d_valid.download((H, W), np.uint16)
    for n_q in arms.values():
        device(n_q)  # warm-up
    runs = {name: [] for name in arms}
    equal = {}
    for _ in range(args.runs):
        for name, n_q in arms.items():  # interleaved
            steps = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                device(n_q)
                steps.append(time.perf_counter() - t0)
            dev_flat = d_flat.download((H, W), np.float32)
            dev_dark = d_dark.download((H, W), np.float32) if n_q == 2 else None
            t0 = time.perf_counter()
            ref_flat, ref_dark = engine.flat_finish_ref(R[:n_q], valid, (H, W), taps, floor)
            t1 = time.perf_counter()
            np_flat, np_dark = numpy_finish(R[:n_q], valid, args.sigma, floor)
            t2 = time.perf_counter()
            equal[name] = bool(dev_flat.tobytes() == ref_flat.tobytes() and (n_q == 1 or dev_dark.tobytes() == ref_dark.tobytes()))
            close = bool(np.all(np.abs(dev_flat.astype(np.float64) - np_flat) <= np.spacing(np.maximum(dev_flat, np_flat))))
            runs[name].append({"device_seconds": round(statistics.median(steps), 6), "device_step_seconds": [round(t, 6) for t in steps],
                               "host_build_seconds": round(t1 - t0, 4), "numpy_seconds": round(t2 - t1, 4),
                               "device_equals_host_build": equal[name], "within_one_float32_spacing_of_numpy": close})  # fmt: skip
    result = {"tool": "tools/bench_flat_estimation.py --finish",
              "workload": "finish of the rank planes (500, 50) of {} x {} x {} uint16 planes of synth, sigma {} (radius {}), floor {}; "
                          "device: wall clock of DestripeEngine.flat_finish with its buffers given; host build and NumPy on one "
                          "thread of the same machine".format(n, H, W, args.sigma, r, floor), "arms": {}}  # fmt: skip
    for name, n_q in arms.items():
        med = {k: statistics.median(x[k] for x in runs[name]) for k in ("device_seconds", "host_build_seconds", "numpy_seconds")}
        result["arms"][name] = {"n_q": n_q, "runs": runs[name], "median": {k: round(v, 6) for k, v in med.items()},
                                "device_over_host_build": round(med["host_build_seconds"] / med["device_seconds"], 1),
                                "device_over_numpy": round(med["numpy_seconds"] / med["device_seconds"], 1),
                                "host_build_over_numpy": round(med["numpy_seconds"] / med["host_build_seconds"], 2)}  # fmt: skip
    for d in (d_rank, d_valid, d_flat, d_dark, d_work):
        d.free()
    if args.channel_tiles > 0:
        with tempfile.TemporaryDirectory() as tmp:
            result["estimate_channel_flats"] = channel_arm(args, tmp)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


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
    ap.add_argument("--finish", action="store_true", help="bench the finish of the flat instead of the rank kernel")
    ap.add_argument("--sigma", type=float, default=32.0)
    ap.add_argument("--channel-tiles", type=int, default=2, help="tiles of the estimate_channel_flats arm (0: leave it out)")
    ap.add_argument("--channel-planes", type=int, default=8)
    args = ap.parse_args()
    n, H, W = args.planes, args.height, args.width
    P = H * W
    bank = synth.synthetic_bank(min(32, n), H, W)
    eng = engine.DestripeEngine(0)
    d_stack = eng.alloc(2 * n * P)
    for z in range(n):  # synth.synthetic_stack, plane by plane
        d_stack.upload(np.roll(bank[z % len(bank)], z // len(bank), axis=0), offset=2 * z * P)
    if args.finish:
        finish_bench(args, eng, d_stack, n, H, W)
        d_stack.free()
        eng.close()
        return
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
