"""What ``rotate=True`` costs, and that ``rotate=False`` costs nothing: the log-space chain over device-resident planes
(uint16 in, uint16 out, production configs, one cohort of ``--batch`` planes as ``bench.py`` runs it) with the option
off and on, ``--runs`` interleaved runs per arm in one session, medians.  With ``--parent-root DIR`` (a built checkout
of the commit before the option existed) a third arm runs that tree's library and package the same way, interleaved
with the other two: the off arm has to lie inside the spread of its runs, and its output bytes have to be the same.

The order of the arms moves on by one per run (parent, off, on; off, on, parent; ...): with a fixed order the arm that
always ran first, behind the idle gap between runs, measured about 1 % slower than the same code run second.

Every arm is a child process of its own (a fresh context, its own planes in device memory) that stays up for the whole
measurement and runs one timed burst whenever it is told to, so only one arm uses the GPU at a time.

    python tools/bench_rotate.py [--parent-root DIR] [--bench] --out profiles/rotate_bench.json

``--bench`` also runs ``python bench.py --gpus 1`` in the same session and stores its result line next to the arms.
The on arm adds two streaming passes over the planes (read + write of the input planes going in, of the result planes
coming out): 4 x 2 bytes per pixel on top of what the chain moves, which the record states next to the measured ratio.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import sys, zlib
root, H, W, batch, steps, warmup, arm = sys.argv[1], *map(int, sys.argv[2:7]), sys.argv[7]
sys.path.insert(0, root)
import numpy as np
from aind_smartspim_destripe_amd import engine as E, synth
e = E.DestripeEngine(0)
kw = {} if arm == "parent" else {"rotate": arm == "on"}
e.plan(H, W, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=batch, **kw)
stack = synth.synthetic_stack(batch, H, W, bank=synth.synthetic_bank(min(32, batch), H, W))
d_in, d_out, d_cfg = e.alloc(stack.nbytes), e.alloc(stack.nbytes), e.alloc(4 * batch)
d_in.upload(stack)
for _ in range(warmup):
    e.run_device(d_in, np.uint16, batch, d_out, np.uint16, d_cfg)
e.sync()
crc = zlib.crc32(d_out.download(stack.shape, np.uint16).tobytes())
print("ready", crc, flush=True)
for line in sys.stdin:
    if line.strip() != "go":
        break
    e.timer_start()
    for _ in range(steps):
        e.run_device(d_in, np.uint16, batch, d_out, np.uint16, d_cfg)
    print(e.timer_stop() / steps, flush=True)
e.close()
"""


class Arm:
    def __init__(self, name, root, shape, args):
        self.name, self.ms = name, []
        env = {k: v for k, v in os.environ.items() if k != "DSX_LIB"}
        self.proc = subprocess.Popen(
            [sys.executable, "-c", WORKER, root, str(shape[0]), str(shape[1]), str(args.batch), str(args.steps),
             str(args.warmup), name], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root, env=env)  # fmt: skip

    def wait_ready(self):
        line = self.proc.stdout.readline().split()
        if len(line) != 2 or line[0] != "ready":
            raise RuntimeError("arm {} did not come up (exit {})".format(self.name, self.proc.poll()))
        self.crc = int(line[1])

    def burst(self):
        self.proc.stdin.write("go\n")
        self.proc.stdin.flush()
        line = self.proc.stdout.readline()
        if not line.strip():
            raise RuntimeError("arm {} ended (exit {})".format(self.name, self.proc.poll()))
        self.ms.append(float(line))

    def close(self):
        try:
            self.proc.stdin.close()
        except OSError:
            pass
        self.proc.wait(timeout=120)


def measure(shape, args):
    roots = [("off", REPO), ("on", REPO)]
    if args.parent_root:
        roots.insert(0, ("parent", os.path.abspath(args.parent_root)))
    arms = []
    try:
        for name, root in roots:  # one after the other: a failed start ends the measurement before the next one begins
            arm = Arm(name, root, shape, args)
            arms.append(arm)
            arm.wait_ready()
        for r in range(args.runs):  # the order moves on by one arm per run, so that no arm always follows the same one
            for k in range(len(arms)):
                arms[(k + r) % len(arms)].burst()
    finally:
        for arm in arms:
            arm.close()
    by = {a.name: a for a in arms}
    H, W = shape
    rec = {"shape": [H, W], "planes": args.batch, "steps_per_run": args.steps,
           "ms_per_cohort": {a.name: a.ms for a in arms},
           "median_ms": {a.name: statistics.median(a.ms) for a in arms}}  # fmt: skip
    off, on = rec["median_ms"]["off"], rec["median_ms"]["on"]
    rec["on_over_off"] = on / off
    # the two turns: the input planes read and written once more, and the result planes
    extra = 4 * 2 * H * W
    rec["extra_bytes_per_plane"] = extra
    rec["added_us_per_plane"] = (on - off) * 1e3 / args.batch
    rec["added_passes_gb_per_s"] = extra * args.batch / ((on - off) * 1e-3) / 1e9 if on > off else None
    if "parent" in by:
        lo, hi = min(by["parent"].ms), max(by["parent"].ms)
        rec["parent_spread_ms"] = [lo, hi]
        rec["off_inside_parent_spread"] = bool(lo <= off <= hi)
        rec["off_bytes_equal_parent"] = bool(by["off"].crc == by["parent"].crc)
    else:
        rec["parent_spread_ms"] = "not measured"
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="2048x2048,1600x2000")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20, help="cohorts per timed run")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="built checkout of the parent commit (third arm)")
    ap.add_argument("--bench", action="store_true", help="also run bench.py --gpus 1 in this session")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tool": "tools/bench_rotate.py", "date": time.strftime("%Y-%m-%d"), "arms": []}
    for s in args.shapes.split(","):
        shape = tuple(int(v) for v in s.lower().split("x"))
        rec = measure(shape, args)
        print(json.dumps(rec), flush=True)
        result["arms"].append(rec)
    if args.bench:
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"], cwd=REPO, capture_output=True,
                           text=True, timeout=900)  # fmt: skip
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        result["bench_py"] = json.loads(lines[-1]) if r.returncode == 0 and lines else "failed (exit {})".format(r.returncode)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
