#!/usr/bin/env python3
"""The launch chain of every branch of run_cohort (csrc/dsx.hip), case by case: which kernels are dispatched with what
grid, block and LDS size, and a CRC32 of what they compute.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/chain_trace.py run OUT.json
        runs CASES through the public engine API, one engine per case (the case's switches are put into the environment
        before the engine is created: dsx_init reads them per context), a warm-up call before the traced ones; OUT.json
        gets the CRC32 of each case's result bytes and cfg_used, and the CU count of the device.  The traced calls of a
        case sit between two marker dispatches (k_downsample2 with the case number in its grid).
    python tools/chain_trace.py parse DIR RUN.json OUT.json
        the dispatches of each case (name with template arguments, grid in blocks, workgroup size, LDS bytes, queue) in
        dispatch order, from the kernel trace under DIR, joined with the CRCs of RUN.json
    python tools/chain_trace.py compare A.json B.json
        per case: same dispatch sequence? same sequence per queue? same multiset? same CRCs?  Exit status 1 on a difference.
    python tools/chain_trace.py golden A.json tests/golden/chain_launches.json
        the chain kernels' launches per case and the CU count they were recorded on, for tests/test_chain_host.py

CASES covers every branch of the chain at the smallest shape that reaches it (plans checked with
tests/host/dsx_host_check plan); tests/test_chain_host.py runs the same table through dsx_chain.h on the CPU.
"""
import collections
import csv
import glob
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the kernels run_cohort launches (a trace holds others: the markers, the band / blend kernels of the dual-band filter)
CHAIN_KERNELS = ("k_zero3", "k_fwd_march", "k_fwd_gen", "k_hist", "k_otsu", "k_rowfilter", "k_rowfinal", "k_inv_march",
                 "k_inv_gen")
SWITCHES = ("DSX_SEG_MIN_ROWS", "DSX_MARCH_WAVES", "DSX_FWD_WPB", "DSX_INV_WPB", "DSX_ROW_WPB", "DSX_HIST_ROWS", "DSX_STREAMS",
            "DSX_HELPER", "DSX_NO_QUANT", "DSX_NO_ROW_MULTI", "DSX_ROW_MULTI_ALONE", "DSX_NO_PAIR", "DSX_NO_FUSE",
            "DSX_NO_FUSE_INV", "DSX_NO_FUSE_RF", "DSX_FUSE_RF_WIDE", "DSX_NO_PIPELINE", "DSX_GRAPH", "DSX_PRIO",
            "DSX_NO_ROW_PACK", "DSX_ROW_PACK", "DSX_ROW_PACK_WPB", "DSX_ROW_PACK_FILL")


def _case(name, H, W, n, in_dt="uint16", out_dt="uint16", env=None, **kw):
    c = {"name": name, "H": H, "W": W, "n": n, "in": in_dt, "out": out_dt, "env": dict(env or {}), "warm": 1, "calls": 1,
         "out_offset": 0, "level": None, "wavelet": "db3", "stack": False, "streaks": False}
    c.update(kw)
    return c


def _cases():
    t = []
    for n in (1, 5, 64):  # k_rowfinal, plans 1026 = 19.9.6 and 1071 = 17.9.7; 64 planes: 4 parts of 16
        t.append(_case("64x2048_n%d" % n, 64, 2048, n))
    t.append(_case("64x2048_u16_f32", 64, 2048, 5, out_dt="float32"))  # no k_rowfinal
    t.append(_case("64x2048_f32_f32", 64, 2048, 5, in_dt="float32", out_dt="float32"))  # no pair I/O either
    t.append(_case("64x2048_result_off2", 64, 2048, 5, out_offset=2))
    for w in (2000, 1800):  # plans 2048 = 16.16.8 / 1024 = 16.8.8 and 1815 = 15.11.11 / 960 = 15.8.8
        t.append(_case("64x%d" % w, 64, w, 5))
        t.append(_case("64x%d_rf_wide" % w, 64, w, 5, env={"DSX_FUSE_RF_WIDE": 1}))
    t.append(_case("40x4800", 40, 4800, 2))  # k_rowfilter_wide at levels 1, 2; generic CPL 36 at level 3
    t.append(_case("50x70", 50, 70, 3))      # width no multiple of 4: nothing fused
    t.append(_case("33x47", 33, 47, 3))      # odd on both axes, padded result, L = 2
    for n in (1, 48, 49):                    # L = 5; 48 / 49 straddle row_multi_alone
        t.append(_case("256x256_n%d" % n, 256, 256, n))
    t.append(_case("512x2048_n16", 512, 2048, 16))  # march_segments: the quantisation score decides
    t.append(_case("2048x2048_n8", 2048, 2048, 8))
    t.append(_case("96x128_level0", 96, 128, 3, level=0))
    t.append(_case("96x128_haar", 96, 128, 3, wavelet="haar"))
    t.append(_case("96x128_db5", 96, 128, 3, wavelet="db5"))
    t.append(_case("64x128_stack", 64, 128, 3, stack=True))
    t.append(_case("128x128_streaks_march", 128, 128, 2, streaks=True))
    one = [("DSX_NO_FUSE", 1), ("DSX_NO_FUSE_INV", 1), ("DSX_NO_PAIR", 1), ("DSX_NO_FUSE_RF", 1), ("DSX_NO_ROW_MULTI", 1),
           ("DSX_NO_QUANT", 1), ("DSX_FWD_WPB", 4), ("DSX_INV_WPB", 4), ("DSX_ROW_WPB", 4), ("DSX_ROW_WPB", 8),
           ("DSX_HIST_ROWS", 1), ("DSX_HIST_ROWS", 256), ("DSX_MARCH_WAVES", 64), ("DSX_MARCH_WAVES", 16384),
           ("DSX_SEG_MIN_ROWS", 2), ("DSX_SEG_MIN_ROWS", 24), ("DSX_ROW_MULTI_ALONE", 0), ("DSX_HELPER", 0), ("DSX_HELPER", 1)]
    for H, W in ((256, 256), (64, 2048)):
        for k, v in one:
            t.append(_case("%dx%d_%s=%s" % (H, W, k, v), H, W, 5, env={k: v}))
        # three calls: eager, capture + launch, replay
        t.append(_case("%dx%d_DSX_GRAPH=1" % (H, W), H, W, 5, env={"DSX_GRAPH": 1}, warm=0, calls=3))
    t.append(_case("64x2048_n64_DSX_STREAMS=1", 64, 2048, 64, env={"DSX_STREAMS": 1}))
    t.append(_case("64x2048_n64_DSX_STREAMS=2", 64, 2048, 64, env={"DSX_STREAMS": 2}))
    t.append(_case("64x2048_n64_DSX_NO_PIPELINE=1", 64, 2048, 64, env={"DSX_NO_PIPELINE": 1}, warm=0, calls=2))
    return t


CASES = _cases()


def host_check_args(c, cus):
    """Arguments of the ``chain`` mode of tests/host/dsx_host_check for a case (its switches go into the environment)."""
    from aind_smartspim_destripe_amd import wavelets

    n, level = c["n"], -1 if c["level"] is None else c["level"]
    a = {"H": c["H"], "W": c["W"], "n": n, "max_batch": n, "in_u16": int(c["in"] == "uint16"), "out_u16": int(c["out"] == "uint16"),
         "out_off": c["out_offset"], "stack": int(c["stack"]), "calls": c["calls"], "cus": cus, "l0": level, "l1": level,
         "flen": 0 if c["wavelet"] == "db3" else len(wavelets.filter_bank(c["wavelet"])[0]),
         "streams": max(1, min(int(c["env"].get("DSX_STREAMS", 4)), 8))}
    if c["streaks"]:  # the chain runs over the two band planes of every plane and writes float32 bands
        a.update(n=2 * n, max_batch=2 * n, out_u16=0, st_march=1)
    return ["%s=%s" % kv for kv in a.items()]


class _At:
    """A device address inside a DeviceBuffer (run_device reads ``.ptr`` only)."""

    def __init__(self, buf, offset):
        self.ptr = buf.ptr + offset


def run_case(i, c):
    import numpy as np

    from aind_smartspim_destripe_amd import engine as eng_mod, synth

    for k in SWITCHES:
        os.environ.pop(k, None)
    for k, v in c["env"].items():
        os.environ[k] = str(v)
    e = eng_mod.DestripeEngine(0)
    try:
        H, W, n = c["H"], c["W"], c["n"]
        bank = synth.synthetic_bank(min(n, 8), H, W)
        planes = np.ascontiguousarray(bank[np.arange(n) % bank.shape[0]].astype(c["in"]))
        if c["streaks"]:
            info = e.plan_streaks(H, W, 64.0, 128.0, max_batch=n, route="march")
        else:
            cells = dict(synth.CELLS_CONFIG, wavelet=c["wavelet"], level=c["level"])
            nocells = dict(synth.NO_CELLS_CONFIG, wavelet=c["wavelet"], level=c["level"])
            info = e.plan(H, W, cells, nocells, synth.ZARR_PATH_HIGH_INT, max_batch=n)
            if c["stack"]:
                e.set_stack_mode(True)
        out = np.zeros((n, info.out_height, info.out_width), dtype=c["out"])
        d_in, d_out, d_cfg = e.alloc(planes.nbytes), e.alloc(out.nbytes + 16), e.alloc(4 * n)
        d_mark = e.alloc(64 * 2 * (i + 2) * 2)
        d_in.upload(planes)
        d_out.upload(np.zeros(out.nbytes + 16, dtype=np.uint8))
        d_cfg.upload(np.zeros(n, dtype=np.int32))
        at = _At(d_out, c["out_offset"])
        cfg = None if c["streaks"] else d_cfg
        for _ in range(c["warm"]):
            e.run_device(d_in, planes.dtype, n, at, out.dtype, cfg)
        e.downsample2(d_mark, _At(d_mark, 32 * 2 * (i + 2) * 2), (2, 2 * (i + 1), 2))   # marker: grid (1, i + 1, 1)
        for _ in range(c["calls"]):
            e.run_device(d_in, planes.dtype, n, at, out.dtype, cfg)
        e.downsample2(d_mark, _At(d_mark, 32 * 2 * (i + 2) * 2), (4, 2 * (i + 1), 2))   # marker: grid (1, i + 1, 2)
        e.sync()
        res = d_out.download(out.nbytes, np.uint8, offset=c["out_offset"])
        cfg_used = d_cfg.download(n, np.int32)
        return {"crc_out": zlib.crc32(res.tobytes()), "crc_cfg": zlib.crc32(cfg_used.tobytes())}
    finally:
        e.close()


def cmd_run(out_path):
    res = {"cases": {}}
    for i, c in enumerate(CASES):
        res["cases"][c["name"]] = run_case(i, c)
        print(c["name"], res["cases"][c["name"]], flush=True)
    try:
        import torch

        res["cus"] = int(torch.cuda.get_device_properties(0).multi_processor_count)
        res["device"] = torch.cuda.get_device_name(0)
    except Exception as err:  # noqa: BLE001
        res["cus"], res["device"] = None, repr(err)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def kernel_name(raw):
    """``void dsx::k_rowfilter<18, 4, 1, 0, 1>(dsx::RowArgs)`` -> ``k_rowfilter<18, 4, 1, 0, 1>``"""
    s = raw.strip()
    if s.startswith("void "):
        s = s[5:]
    s = s.replace("(anonymous namespace)::", "").replace("dsx::", "")
    s = s.split("(")[0].strip()
    return s[:-3] if s.endswith(".kd") else s


def cmd_parse(trace_dir, run_path, out_path):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
                grid = [int(r["Grid_Size_" + a]) // max(1, w) for a, w in zip("XYZ", wg)]
                lds = next(int(r[k]) for k in ("LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v") if k in r)
                rows.append((int(r["Dispatch_Id"]), kernel_name(r["Kernel_Name"]), grid, wg[0] * wg[1] * wg[2], lds,
                             r.get("Queue_Id", "")))
    rows.sort()
    run = json.load(open(run_path))
    cases, cur, open_case = {}, None, None
    for _, name, grid, block, lds, queue in rows:
        if name.startswith("k_downsample2"):
            idx = grid[1] - 1
            if grid[2] == 1:
                open_case, cur = CASES[idx]["name"], []
            else:
                assert open_case == CASES[idx]["name"], (open_case, idx)
                cases[open_case] = dict(run["cases"][open_case], dispatches=cur)
                open_case, cur = None, None
        elif cur is not None:
            cur.append([name, grid, block, lds, queue])
    missing = [c["name"] for c in CASES if c["name"] not in cases]
    assert not missing, ("cases without markers in the trace", missing)
    with open(out_path, "w") as f:
        json.dump({"cus": run.get("cus"), "device": run.get("device"), "cases": cases}, f)
    print("parsed %d dispatches, %d cases -> %s" % (len(rows), len(cases), out_path))


def _per_queue(disp):
    q = collections.defaultdict(list)
    for d in disp:
        q[d[4]].append(tuple(map(str, d[:4])))
    return sorted(map(tuple, q.values()))


def cmd_compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    print("A = %s   B = %s" % (a_path, b_path))
    print("%-34s %5s %5s  %-8s %-9s %-8s %-4s" % ("case", "nA", "nB", "sequence", "per-queue", "multiset", "crc"))
    for c in CASES:
        x, y = a["cases"][c["name"]], b["cases"][c["name"]]
        dx, dy = [d[:4] for d in x["dispatches"]], [d[:4] for d in y["dispatches"]]
        seq = dx == dy
        pq = _per_queue(x["dispatches"]) == _per_queue(y["dispatches"])
        ms = sorted(map(str, dx)) == sorted(map(str, dy))
        crc = (x["crc_out"], x["crc_cfg"]) == (y["crc_out"], y["crc_cfg"])
        bad += not (ms and crc and (seq or pq))
        print("%-34s %5d %5d  %-8s %-9s %-8s %-4s  out %08x cfg %08x" % (c["name"], len(dx), len(dy), "same" if seq else "DIFF",
              "same" if pq else "DIFF", "same" if ms else "DIFF", "same" if crc else "DIFF", x["crc_out"], x["crc_cfg"]))
        if not ms:
            for k, (p, q) in enumerate(zip(dx, dy)):
                if p != q:
                    print("    first difference at dispatch %d: %s  |  %s" % (k, p, q))
                    break
    print("%d of %d cases differ" % (bad, len(CASES)))
    return 1 if bad else 0


def cmd_golden(a_path, out_path):
    a = json.load(open(a_path))
    cases = {}
    for c in CASES:
        disp = a["cases"][c["name"]]["dispatches"]
        cases[c["name"]] = [d[:4] for d in disp if d[0].split("<")[0] in CHAIN_KERNELS or d[0].split("<")[0].startswith("k_rowfilter")]
    with open(out_path, "w") as f:
        json.dump({"cus": a["cus"], "launches": cases}, f, separators=(",", ":"))
    print("%d cases -> %s" % (len(cases), out_path))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run":
        cmd_run(sys.argv[2])
    elif cmd == "parse":
        cmd_parse(*sys.argv[2:5])
    elif cmd == "compare":
        sys.exit(cmd_compare(*sys.argv[2:4]))
    elif cmd == "golden":
        cmd_golden(*sys.argv[2:4])
    else:
        sys.exit(__doc__)
