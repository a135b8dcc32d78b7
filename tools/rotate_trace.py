"""Device time of ``k_rot90`` next to ``k_planes_to_bricks`` -- the yardstick: another kernel that only moves uint16
planes -- from ONE ``rocprofv3 --kernel-trace --stats`` run per shape (a run of its own, no counters).

    python tools/rotate_trace.py [--shapes 2048x2048,1600x2000] [--planes 64] > profiles/rotate_kernels.txt

Without ``--run`` the tool starts ``rocprofv3 ... -- python tools/rotate_trace.py --run HxW`` once per shape (a fresh
process each) and prints one table per shape from the trace.  The traced process turns ``--planes`` uint16 planes
stand-alone in both directions (``dsx_rot90_device``, one dispatch each, alone on the device, three times), re-tiles them
into (64, 128, 128) bricks three times, and runs one cohort of a ``rotate=True`` plan (the turns inside the launch chain,
one dispatch per stream part and direction, overlapping the other parts' kernels).  GB/s counts bytes read plus bytes
written.

``--pmc``: instead of the trace, one counter run of its own per shape (``rocprofv3 --pmc SQ_LDS_BANK_CONFLICT
SQ_LDS_IDX_ACTIVE``, no tracing) over the same workload: the LDS cycles of ``k_rot90`` and how many of them are
bank-conflict cycles, summed over its dispatches.
"""

import argparse
import collections
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
BRICK = (64, 128, 128)


def run(shape, planes):
    import numpy as np

    from aind_smartspim_destripe_amd import engine as E
    from aind_smartspim_destripe_amd import synth

    H, W = shape
    e = E.DestripeEngine(0)
    stack = synth.synthetic_stack(planes, H, W, bank=synth.synthetic_bank(min(8, planes), H, W))
    d_a, d_b = e.alloc(stack.nbytes), e.alloc(stack.nbytes)
    nb = [-(-n // c) for n, c in zip((planes, H, W), BRICK)]
    d_bricks = e.alloc(2 * int(np.prod(nb)) * int(np.prod(BRICK)))
    d_a.upload(stack)
    for _ in range(3):
        e.rot90_device(d_a, d_b, np.uint16, planes, H, W, 1)
        e.sync()
        e.rot90_device(d_b, d_a, np.uint16, planes, W, H, -1)
        e.sync()
    for _ in range(3):
        e.planes_to_bricks(d_a, d_bricks, (planes, H, W), BRICK)
        e.sync()
    e.plan(H, W, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=planes, rotate=True)
    for _ in range(2):
        e.run_device(d_a, np.uint16, planes, d_b, np.uint16)
        e.sync()
    e.close()


def table(shape, planes, out_dir):
    H, W = shape
    px = planes * H * W
    nb = [-(-n // c) for n, c in zip((planes, H, W), BRICK)]
    brick_elems = nb[0] * nb[1] * nb[2] * BRICK[0] * BRICK[1] * BRICK[2]
    rows = collections.defaultdict(list)
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "k_rot90" in name or "k_planes_to_bricks" in name:
                key = name.replace("void ", "").replace("dsx::rot::", "").replace("dsx::", "").split("(")[0]
                rows[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("shape {} x {}, {} uint16 planes".format(H, W, planes))
    print("%-44s %9s %12s %12s %10s" % ("kernel", "launches", "median us", "bytes", "GB/s"))
    for key in sorted(rows):
        disp = sorted(rows[key])
        if "k_rot90" in key:
            alone, chain = disp[:3], disp[3:]  # the stand-alone dispatches come first (run above)
            us = sorted(d for _, d in alone)[len(alone) // 2] / 1e3
            print("%-44s %9d %12.1f %12d %10.0f" % (key + " alone", len(alone), us, 4 * px, 4 * px / us / 1e3))
            if chain:
                tot = sum(d for _, d in chain) / 1e3
                nbytes = 2 * 4 * px  # two cohorts of the rotated plan, this direction: read + write of px voxels each
                print("%-44s %9d %12.1f %12d %10.0f   (sum over the stream parts, overlapped with other kernels)"
                      % (key + " in the chain", len(chain), tot, nbytes, nbytes / tot / 1e3))
        else:
            us = sorted(d for _, d in disp)[len(disp) // 2] / 1e3
            nbytes = 2 * px + 2 * brick_elems
            print("%-44s %9d %12.1f %12d %10.0f" % (key, len(disp), us, nbytes, nbytes / us / 1e3))
    print()


def counters(shape, out_dir):
    tot = collections.defaultdict(lambda: collections.Counter())
    for f in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "k_rot90" in name or "k_planes_to_bricks" in name:
                key = name.replace("void ", "").replace("dsx::rot::", "").replace("dsx::", "").split("(")[0]
                tot[key][r["Counter_Name"]] += float(r["Counter_Value"])
    print("shape {} x {}: LDS counters, summed over the dispatches of a kernel".format(*shape))
    for key in sorted(tot):
        c = tot[key]
        active, conflict = c.get("SQ_LDS_IDX_ACTIVE", 0.0), c.get("SQ_LDS_BANK_CONFLICT", 0.0)
        print("%-44s SQ_LDS_IDX_ACTIVE %14.0f   SQ_LDS_BANK_CONFLICT %14.0f   (%.1f %% of the LDS cycles)"
              % (key, active, conflict, 100.0 * conflict / active if active else 0.0))
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="2048x2048,1600x2000")
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--run", default=None, metavar="HxW", help="the traced workload itself")
    ap.add_argument("--pmc", action="store_true", help="a counter run (LDS bank conflicts) instead of the trace")
    args = ap.parse_args()
    if args.run:
        run(tuple(int(v) for v in args.run.lower().split("x")), args.planes)
        return 0
    for s in args.shapes.split(","):
        shape = tuple(int(v) for v in s.lower().split("x"))
        out_dir = tempfile.mkdtemp(prefix="rotate_trace_")
        try:
            how = ["--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"] if args.pmc else ["--kernel-trace", "--stats"]
            r = subprocess.run(["rocprofv3"] + how + ["--output-format", "csv", "-d", out_dir, "--",
                                sys.executable, os.path.abspath(__file__), "--run", s, "--planes", str(args.planes)],
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=400)  # fmt: skip
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                return r.returncode  # nothing more is started on the device after a failed run
            if args.pmc:
                counters(shape, out_dir)
            else:
                table(shape, args.planes, out_dir)
        finally:
            shutil.rmtree(out_dir, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
