#!/usr/bin/env python3
"""Headline benchmark: 2048 x 2048 uint16 slices/s destriped + achieved HBM GB/s (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--shape HxW] [--shading] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times K steps and prints the result line.  --full adds what the headline figure does not
need: the CPU baseline (rank 0 of a one-GPU run) and the output verification below.  --dump-outputs DIR writes what the
last timed step computed as DIR/<name>.npy (see dump_outputs), so that two builds can be compared output for output.

One "step" = one pass of the hot path (filter_stripes semantics, production parameters,
uint16 in -> uint16 out) over a batch of 256 synthetic striped slices that is already resident in
HBM.  N > 1: one rank per GPU, either launched by torch.distributed.run (the launcher only: RANK /
LOCAL_RANK / WORLD_SIZE) or -- when `python bench.py --gpus N` is run by itself, without WORLD_SIZE in
the environment -- started by this script: the parent touches no GPU, starts N child processes of itself
with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* / DSX_RDZV_DIR set, relays rank 0's JSON line and exits
non-zero if any rank does.  Slices shard embarrassingly (weak scaling, 256 slices per rank).  The only collective
is one RCCL broadcast of the filter-constant blob before the timed region; it, the barriers and the
max-over-ranks of the time go straight through the C ABI (dsx_comm_*, librccl.so; no torch).
A failing collective or a result that does not verify ends the run with a non-zero exit code.

With --full, after the timed region the output is VERIFIED: planes 0 and 1 against the reference's golden samples
(tests/golden/large_stats.npz, written by the real reference), and one plane from every sub-cohort
stream part against a single-stream re-run of the same plane (bit-identical), so every stream's output
is tied to the reference.
"""

import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from aind_smartspim_destripe_amd import distributed as dsx_dist  # noqa: E402
from aind_smartspim_destripe_amd import engine as eng_mod  # noqa: E402
from aind_smartspim_destripe_amd import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0
# The attainable fraction of this algorithm in FP32 on gfx950 (derived from numbers in profiles/):
# the chain at its floors -- 3.9 M vector wave-instructions and 50.2 MB of HBM traffic per 2048 x 2048 plane (32.4 read,
# 17.8 written; level 1 materialised once: the decomposition that never materialises it trades 13 MB for + 1.4 M
# instructions and is bound lower, by the vector units) -- needs 7.0 us of vector issue slots and, priced at the
# measured 6.0 TB/s read and 3.5 TB/s write rates of this chip one after the other, 10.5 us of bus time per plane:
# 95 k planes/s = 0.200 of the 8 TB/s data-sheet peak with both bounds perfectly overlapped.  (Reads and writes
# overlap on the bus -- a copy moves 6.2 TB/s in all -- which would put the bound at 8.1 us = 0.259; no kernel pair
# of this chain has been seen to reach that, so the additive figure is the one reported.)
ATTAINABLE_FRAC_2048 = 0.200
ATTAINABLE_FRAC_2048_RW_OVERLAPPED = 0.259
SETTLE_SECONDS = 1.0  # untimed back-to-back steps before the warm-up: the chip reaches its steady clock


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def synthetic_shading(h, w):
    """flat = 1.0 + smooth vignetting, dark = 100."""
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = ((yy - h / 2.0) / (h / 2.0)) ** 2 + ((xx - w / 2.0) / (w / 2.0)) ** 2
    flat = (1.0 - 0.15 * r2).astype(np.float32)
    dark = np.full((h, w), 100.0, dtype=np.float32)
    return flat, dark


def cpu_worker(first, count, start_at, h, w):
    """Child process of the CPU baseline: the NumPy oracle over `count` planes on one thread.  Prints
    "start end" (epoch seconds of its timed region).  Never touches the GPU."""
    from oracle import destripe_oracle as orc

    p = synth.synthetic_plane(0, 256, 256)
    orc.filter_stripes(p, "t", synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, synth.ZARR_PATH_HIGH_INT)  # warm numpy
    planes = [synth.synthetic_plane(k % 32, h, w) for k in range(first, first + count)]
    while time.time() < start_at:  # common start so that the workers really run side by side
        time.sleep(0.01)
    t0 = time.time()
    for p in planes:
        out = orc.filter_stripes(p, "t", synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, synth.ZARR_PATH_HIGH_INT)
        np.clip(out, 0, 65535).astype(np.uint16)
    print("{:.6f} {:.6f}".format(t0, time.time()), flush=True)


def cpu_baseline(n_planes, procs, h, w):
    """The NumPy oracle (a port of the reference algorithm) on the host cores, bounded sample: `procs`
    independent single-thread processes (the reference's execution model, zarr_destriper.py:1151-1165),
    `n_planes` planes in total.  Children are started BEFORE this process initialises the GPU."""
    import subprocess

    procs = max(1, min(procs, n_planes))
    per = n_planes // procs
    start_at = time.time() + 8.0 + 0.5 * per * (h * w) / (2048.0 * 2048.0)  # imports + warm-up + making the planes
    kids = [
        subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(i * per), str(per),
                          repr(start_at), str(h), str(w)],
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        for i in range(procs)
    ]  # fmt: skip
    spans = []
    for k in kids:
        out, _ = k.communicate(timeout=1500)
        if k.returncode != 0:
            raise RuntimeError("cpu baseline worker failed")
        t0, t1 = map(float, out.split()[-2:])
        spans.append((t0, t1))
    wall = max(t1 for _, t1 in spans) - min(t0 for t0, _ in spans)
    busy = sum(t1 - t0 for t0, t1 in spans)
    done = per * procs
    return {
        "value": round(done / wall, 4),
        "unit": "slices/s",
        "cores": procs,
        "kind": "port",
        "per_core": round(done / busy, 4),
        "sample": "{} synthetic {}x{} uint16 planes ({} per process, {} single-thread processes side by side), "
                  "NumPy oracle filter_stripes + uint16 cast, {:.1f} s wall".format(done, h, w, per, procs, wall),
    }  # fmt: skip


def golden_name(h, w):
    return "s{}".format(h) if h == w else "s{}x{}".format(h, w)


def verify(engine, stack, d_out, h, w, batch, cohort, n_streams, shading, wavelet="db3"):
    """Tie the timed configuration's output to the reference.  Returns (ok, details)."""
    details = {}
    ok = True
    out01 = d_out.download((2, h, w), np.uint16)
    gpath = os.path.join(REPO, "tests", "golden", "large_stats.npz")
    flat = dark = None
    if shading is not None:
        flat, dark = shading
    # (1) planes 0, 1 (= bank planes 0, 1) against the real reference's samples.  With shading on, the
    # reference's float result is pushed through flatfield_correction's arithmetic first (filtering.py:399-412).
    if os.path.exists(gpath):
        g = np.load(gpath, allow_pickle=False)
        name = golden_name(h, w)
        if name + "__k0__u16__sample" in g.files and wavelet == "db3":
            rs = np.random.RandomState(7)
            sy, sx = rs.randint(0, h, 4096), rs.randint(0, w, 4096)
            worst, n_off = 0, 0
            for k in (0, 1):
                ref = g["{}__k{}__u16__sample".format(name, k)]
                if shading is not None:
                    d = dark[sy, sx].astype(np.float64)
                    ref = np.where(ref > d, ref - d, 0.0) / flat[sy, sx].astype(np.float64)
                want = np.clip(ref, 0, 65535).astype(np.uint16).astype(np.int64)
                got = out01[k][sy, sx].astype(np.int64)
                diff = np.abs(got - want)
                # truncation to uint16 is discontinuous: a float32 result within 1e-4 of an integer may land
                # one count away; a sample under a flipped mask coefficient (<= 2 of 4096) may be further off
                n_far = int((diff > np.maximum(1, 2e-4 * want)).sum())
                n_off += int((diff > 0).sum())
                worst = max(worst, int(diff.max()))
                if n_far > 2 or diff.max() > 0.05 * want.max():
                    ok = False
            details["golden_planes"] = [0, 1]
            details["golden_samples_off_by_one"] = n_off
            details["golden_worst_count_diff"] = worst
        else:
            details["golden_planes"] = "no golden vector for this shape / wavelet"
    # (2) one plane of every stream part, re-run alone on the main stream: must be bit-identical
    parts = n_streams
    nb = min(cohort, batch)
    while parts > 1 and nb // parts < 16:
        parts -= 1
    per = (nb + parts - 1) // parts
    picks = sorted({min(nb - 1, i * per + (7 * i + 3) % max(per, 1)) for i in range(parts)} | {batch - 1})
    d_one_in = engine.alloc(2 * h * w * 2)
    d_one_out = engine.alloc(2 * h * w * 2)
    try:
        for z in picks:
            d_one_in.upload(np.ascontiguousarray(stack[[z, 1]]))
            engine.run_device(d_one_in, np.uint16, 2, d_one_out, np.uint16, None)
            engine.sync()
            alone = d_one_out.download((1, h, w), np.uint16)[0]
            timed = d_out.download((1, h, w), np.uint16, offset=z * h * w * 2)[0]
            if not np.array_equal(alone, timed):
                ok = False
                details.setdefault("stream_part_mismatch", []).append(int(z))
    finally:
        d_one_in.free()
        d_one_out.free()
    details["stream_part_planes_bit_identical"] = [int(z) for z in picks]
    details["stream_parts"] = parts
    return ok, details


DUMP_SLICES_BYTES = 32 << 20  # whole slices
DUMP_SAMPLE_BYTES = 16 << 20  # the same seeded pixels of every slice


def dump_outputs(out_dir, d_out, cfg, h, w, batch):
    """What a caller of the timed path receives -- the uint16 slices and the config each slice was filtered with --
    written as float32 .npy files (48 MiB in all at most; every uint16 value is exact in float32), positions as float64:

      config.npy        [batch]        0 = no-cells config, 1 = cells config
      slices.npy        [k, H, W]      whole slices at slice_index.npy (k evenly spaced slices, first and last included)
      sample.npy        [batch, S]     every slice at the S flat pixel positions of sample_index.npy (seed 0)

    The selection depends on (batch, H, W) only, so two runs with the same arguments dump the same positions."""
    os.makedirs(out_dir, exist_ok=True)
    k = min(batch, DUMP_SLICES_BYTES // (4 * h * w))
    slice_index = np.unique(np.linspace(0, batch - 1, k).round().astype(np.int64)) if k > 0 else np.zeros(0, np.int64)
    n_sample = max(1, min(h * w, DUMP_SAMPLE_BYTES // (4 * batch + 8)))  # sample.npy + sample_index.npy
    sample_index = np.sort(np.random.RandomState(0).choice(h * w, n_sample, replace=False))
    slices = np.empty((len(slice_index), h, w), np.float32)
    sample = np.empty((batch, n_sample), np.float32)
    for z in range(batch):
        plane = d_out.download((h, w), np.uint16, offset=z * h * w * 2)
        sample[z] = plane.reshape(-1)[sample_index]
        hit = np.flatnonzero(slice_index == z)
        if hit.size:
            slices[hit[0]] = plane
    np.save(os.path.join(out_dir, "config.npy"), np.asarray(cfg, np.float32))
    np.save(os.path.join(out_dir, "slices.npy"), slices)
    np.save(os.path.join(out_dir, "slice_index.npy"), slice_index.astype(np.float64))
    np.save(os.path.join(out_dir, "sample.npy"), sample)
    np.save(os.path.join(out_dir, "sample_index.npy"), sample_index.astype(np.float64))


def requested_gpus(argv):
    """--gpus N of the command line (without building the whole parser: the launcher path runs before anything else)."""
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return int(argv[i + 1])
        if a.startswith("--gpus="):
            return int(a.split("=", 1)[1])
    return 1


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script (fresh processes; this parent never
    loads the library or touches a GPU), relay rank 0's stdout (the JSON line), and return the worst exit code.  A rank
    that fails takes the others down after a grace period (they may be waiting for it in a rendezvous)."""
    import socket
    import subprocess
    import tempfile

    with socket.socket() as sk:  # a free port for MASTER_PORT (rendezvous tag; nothing listens on it)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    rdzv = tempfile.mkdtemp(prefix="dsx_rdzv_bench_")  # private (0700), ours
    kids = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DSX_RDZV_DIR=rdzv,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))  # fmt: skip
        kids.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                     stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))  # fmt: skip
    log("[bench] launcher: started {} ranks (pids {}), rendezvous {}".format(n, [k.pid for k in kids], rdzv))
    codes = [None] * n
    first_failure = None
    out0 = b""
    try:
        while any(c is None for c in codes):
            for i, k in enumerate(kids):
                if codes[i] is None and k.poll() is not None:
                    codes[i] = k.returncode
                    if i == 0:
                        out0 = k.stdout.read()
                    if k.returncode != 0 and first_failure is None:
                        first_failure = time.time()
                        log("[bench] launcher: rank {} exited with code {}".format(i, k.returncode))
            if first_failure is not None and time.time() - first_failure > 20.0:
                for i, k in enumerate(kids):  # exactly the processes started above
                    if codes[i] is None:
                        k.kill()
            time.sleep(0.05)
    finally:
        for i, k in enumerate(kids):
            if k.poll() is None:
                k.kill()
        try:
            for f in os.listdir(rdzv):
                os.remove(os.path.join(rdzv, f))
            os.rmdir(rdzv)
        except OSError:
            pass
    sys.stdout.buffer.write(out0)
    sys.stdout.flush()
    bad = [c for c in codes if c != 0]
    return 0 if not bad else (bad[0] if bad[0] and bad[0] > 0 else 1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        return cpu_worker(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    if "WORLD_SIZE" not in os.environ and requested_gpus(sys.argv[1:]) > 1:
        sys.exit(launch_ranks(requested_gpus(sys.argv[1:]), sys.argv[1:]))
    # Only the JSON line may reach stdout: library banners (RCCL) are written to fd 1 directly,
    # so fd 1 is pointed at stderr for the duration of the run and the line goes to the saved fd.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (default: about one second)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256, help="slices per step per GPU")
    ap.add_argument("--shape", default="2048x2048", help="plane shape HxW (BASELINE configs: 2048x2048, 1800x1800, 1600x2000)")
    ap.add_argument("--shading", action="store_true", help="dark / flat-field correction fused into the last kernel")
    ap.add_argument("--wavelet", default="db3", help="wavelet of both configs (db3 = production, specialised kernels; "
                    "any other PyWavelets name runs the tap-count-generic level kernels; not the headline metric)")
    ap.add_argument("--cohort", type=int, default=int(os.environ.get("DSX_COHORT", "256")),
                    help="planes per launch chain (workspace size)")  # fmt: skip
    ap.add_argument("--full", action="store_true",
                    help="also run the CPU baseline and verify the output (a plain run only times the steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (rank 0)")
    ap.add_argument("--cpu-planes", type=int, default=None,
                    help="with --full: planes of the CPU baseline sample (default: 16 per process; 0 = skip)")
    ap.add_argument("--cpu-procs", type=int, default=min(16, os.cpu_count() or 1),
                    help="with --full: single-thread oracle processes of the CPU baseline")
    ap.add_argument("--kernel-breakdown", action="store_true", help="one extra untimed step with per-kernel events")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the output verification (profiling runs)")
    ap.add_argument("--settle", type=float, default=SETTLE_SECONDS,
                    help="seconds of untimed back-to-back steps before the warm-up (0 for profiler runs)")
    args = ap.parse_args()
    H, W = (int(x) for x in args.shape.lower().split("x"))
    algo_bytes_per_slice = H * W * 2 * 2  # compulsory traffic: uint16 read + uint16 write

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # DSX_SHARE_GPU=1 (rehearsal of the multi-rank launch on a box with fewer GPUs than ranks): ranks share the
    # devices round robin.  RCCL refuses two ranks on one GPU, so such a run also exercises the agreed host transport.
    shared_gpu = False
    if os.environ.get("DSX_SHARE_GPU") == "1":
        ndev = int(eng_mod.load_library().dsx_device_count())
        if ndev > 0:
            local, shared_gpu = local % ndev, world > ndev
    if world != args.gpus:
        log("[bench] WORLD_SIZE {} != --gpus {}; using WORLD_SIZE".format(world, args.gpus))

    # CPU baseline first (rank 0, N = 1): its workers are spawned, which must not happen once this process holds the GPU
    cpu = None
    if args.full and world == 1 and args.cpu_planes != 0 and args.wavelet == "db3":
        cpu = cpu_baseline(args.cpu_planes or 16 * args.cpu_procs, args.cpu_procs, H, W)
        log("[bench] cpu baseline: {}".format(cpu))

    engine = eng_mod.DestripeEngine(local)
    shading = synthetic_shading(H, W) if args.shading else None
    info = engine.plan(H, W, dict(synth.CELLS_CONFIG, wavelet=args.wavelet), dict(synth.NO_CELLS_CONFIG, wavelet=args.wavelet),
                       synth.ZARR_PATH_HIGH_INT,
                       max_batch=min(args.cohort, args.batch),
                       flatfield=None if shading is None else shading[0],
                       darkfield=None if shading is None else shading[1])  # fmt: skip
    # N > 1: RCCL communicator + the one collective of the path.  A broadcast that delivers wrong bytes raises
    # (non-zero exit).  If the communicator cannot be built at all, the ranks agree to reduce the timings on the host
    # (the data path has no collective) and the line says so: config.rank_transport = "host" + the reason.
    group = dsx_dist.RankGroup(engine, rank, world)
    blob_bytes = group.broadcast_constants(root=0)
    if world > 1 and group.transport == "rccl":
        log("[bench] rank {}: constants broadcast over RCCL, {} bytes, verified against the local plan".format(rank, blob_bytes))
    elif world > 1:
        log("[bench] rank {}: NO RCCL communicator ({}); barrier / max-over-ranks on the host".format(rank, group.comm_error))

    # synthetic stack: 32 unique planes, slice z = bank[z % 32] rolled by z // 32 rows
    t0 = time.perf_counter()
    bank = synth.synthetic_bank(min(32, args.batch), H, W)
    stack = synth.synthetic_stack(args.batch, H, W, bank=bank)
    log("[bench] rank {} synthetic stack {} in {:.1f} s".format(rank, stack.shape, time.perf_counter() - t0))
    d_in = engine.alloc(stack.nbytes)
    d_out = engine.alloc(stack.nbytes)
    d_cfg = engine.alloc(4 * args.batch)
    d_in.upload(stack)

    def step():
        engine.run_device(d_in, np.uint16, args.batch, d_out, np.uint16, d_cfg)

    def barrier():
        engine.sync()
        group.barrier()

    # settle: untimed, declared in config.settle_steps
    settle_steps = 0
    t_settle = time.perf_counter()
    while time.perf_counter() - t_settle < args.settle:
        step()
        engine.sync()
        settle_steps += 1
    for _ in range(args.warmup):
        step()
    barrier()
    t_start = time.perf_counter()
    engine.timer_start()
    for _ in range(args.steps):
        step()
    dev_ms = engine.timer_stop()  # HIP events on the engine stream; also synchronises it
    barrier()
    wall = time.perf_counter() - t_start
    wall, dev_ms = group.allreduce([wall, dev_ms], "max")

    cfg = d_cfg.download((args.batch,), np.int32)
    n_cells = int(cfg.sum())
    n_streams = int(os.environ.get("DSX_STREAMS", "4"))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, d_out, cfg, H, W, args.batch)
    verified, vdetails = (None, {"skipped": True})
    if args.full and not args.no_verify:
        verified, vdetails = verify(engine, stack, d_out, H, W, args.batch, min(args.cohort, args.batch), n_streams, shading, args.wavelet)
        verified = bool(group.allreduce([1.0 if verified else 0.0], "min")[0] == 1.0)

    breakdown = None
    if args.kernel_breakdown and rank == 0:
        engine.profile(True)
        step()
        engine.sync()
        breakdown = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in engine.profile_read().items()}
        engine.profile(False)

    if rank == 0:
        slices = args.batch * world * args.steps
        value = slices / wall
        ms_per_step = 1e3 * wall / args.steps
        dev_ms_per_step = dev_ms / args.steps
        achieved = args.batch * algo_bytes_per_slice / (dev_ms_per_step * 1e-3) / 1e9
        # HBM bytes per launch chain from the PMC counters: rocprofv3 FETCH_SIZE / WRITE_SIZE passes of
        # tools/traffic.sh on this bench, corrected as MI355X_MICROARCH.md prescribes.  The figure is a
        # property of a BUILD: it is reported only when the profile names this configuration, with its source.
        # The profile carries the sha256 of the native sources it was measured on (build_hash, __graft_entry__.
        # source_hash); the loaded library carries the same stamp (libdsx_hip.so.srchash): no match, no figure.
        traffic, traffic_source = None, None
        try:
            with open(eng_mod.LIB_PATH + ".srchash") as f:
                lib_hash = f.read().strip()
        except OSError:
            lib_hash = None
        for name in sorted(os.listdir(os.path.join(REPO, "profiles")), reverse=True):
            if name.endswith("_traffic.json"):
                with open(os.path.join(REPO, "profiles", name)) as f:
                    t = json.load(f)
                if t.get("planes_per_step") == args.batch and t.get("shape", "2048x2048") == "{}x{}".format(H, W) \
                        and bool(t.get("shading", False)) == bool(args.shading) and args.wavelet == "db3":
                    if lib_hash is not None and t.get("build_hash") == lib_hash:
                        traffic = int(t["hbm_bytes_per_step"])
                        traffic_source = "profiles/{} (build_hash {} = the loaded library)".format(name, lib_hash[:12])
                    else:
                        traffic_source = "profiles/{} was measured on another build (hash {}, library {}): not reported".format(
                            name, str(t.get("build_hash"))[:12], str(lib_hash)[:12])
                    break
        attainable_applies = (H, W) == (2048, 2048) and args.wavelet == "db3" and not args.shading
        result = {
            "metric": "{}x{} uint16 slices/s destriped".format(H, W),
            "value": round(value, 2),
            "unit": "slices/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "verified": verified,
            "config": {
                "workload": "batch of {} x {}x{} uint16 slices per GPU, log-space wavelet-FFT destripe "
                            "(filter_stripes semantics, production cells/no-cells configs, high_int 2500{}{}), "
                            "uint16 out, inputs resident in HBM".format(
                                args.batch, H, W, ", dark/flat-field correction on" if args.shading else "",
                                "" if args.wavelet == "db3" else ", wavelet {} instead of db3".format(args.wavelet)),
                "slices_per_gpu": args.batch,
                "cohort": min(args.cohort, args.batch),
                "sub_cohort_streams": n_streams,
                "levels": info.levels,
                "fft_len": [info.fft_len[i] for i in range(info.levels)],
                "planes_with_cells_config": n_cells,
                "parallelism": "z-sharded x{}".format(world),
                "rccl_ranks": world if group.transport == "rccl" else 0,
                "rank_transport": group.transport,
                "ranks_share_gpus": shared_gpu,
                "rccl_error": group.comm_error,
                "constants_broadcast_bytes": blob_bytes,
                "settle_steps": settle_steps,
                "verification": vdetails,
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "destripe launch chain over one batch: k_fwd_march<u16, fused levels 1 + 2> -> coarse k_fwd_march x6 -> "
                          "k_hist -> k_otsu -> k_rowfilter (levels 2 .. 8) -> k_inv_march x6 -> k_rowfinal (level-1 row filter + "
                          "final synthesis: the dominant kernel, 53 % of a stream's time)",
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5),
                "traffic": traffic,
                "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": args.batch * algo_bytes_per_slice,
                "device_ms_per_launch": round(dev_ms_per_step, 4),
                "read_only_frac": round(achieved / 2 / HBM_PEAK_GBS, 5),
                # what this algorithm can reach in FP32 on this chip (model: DESIGN.md section 4.4; 2048 x 2048, db3, no shading)
                "attainable_frac": ATTAINABLE_FRAC_2048 if attainable_applies else None,
                "frac_of_attainable": round(achieved / HBM_PEAK_GBS / ATTAINABLE_FRAC_2048, 4) if attainable_applies else None,
                "attainable_frac_if_reads_and_writes_overlap": ATTAINABLE_FRAC_2048_RW_OVERLAPPED if attainable_applies else None,
                "attainable_model": "DESIGN.md section 4.4: floors of the chain (3.9 M vector wave-instructions, 32.4 MB read + "
                                    "17.8 MB written per plane) at 6.0 TB/s read, 3.5 TB/s write (measured), 4 clocks per "
                                    "wave-instruction; the bus bound (10.5 us per plane) is the larger" if attainable_applies else None,
            },
        }
        if breakdown is not None:
            result["kernel_ms"] = breakdown
        if cpu is not None:
            result["cpu_baseline"] = cpu
        os.write(json_fd, (json.dumps(result) + "\n").encode())

    d_in.free()
    d_out.free()
    d_cfg.free()
    group.close()
    engine.close()
    if verified is False:
        log("[bench] VERIFICATION FAILED: {}".format(vdetails))
        sys.exit(3)


if __name__ == "__main__":
    main()
