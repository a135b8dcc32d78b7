#!/usr/bin/env python3
"""End-to-end chunk map throughput: an uncompressed uint16 Zarr-v2 store of N planes
2048 x 2048, chunks (1,1,64,128,128), through destripe_zarr (device re-tiling, overlapped upload / filter /
download) into another store.  Prints one JSON line; the roofline of this path is the host link
(PCIe Gen5 x16, 63 GB/s spec: 16.8 MB per plane both ways -> <= 3.7 k planes/s), not HBM.

    bench_zarr.py N [raw|zlib|blosc] [device-codec|device-codec-runs] [device-decode|device-decode-any|device-decode-all]
                  [lz4|blosc-zlib|blosc-blosclz|plain-zlib] [pyramid|fused-pyramid|pipelined-pyramid] [lz4-out] [read-back]
                  [streaks|streaks-generic|streaks-march] [ome-percentile] [scale-FZ-FY-FX] [projections|projections-both]
                  [digests] [store-sha]

`device-codec` (Blosc only): the output chunks are encoded on the GPU (destripe_zarr_store(device_codec=True)); the
line then also reports the bytes written and their ratio to the host writer's frames of the same chunks (first block).
`device-codec-runs`: the same with runs of equal bytes written as matches (device_codec="runs").
`device-decode` (Blosc only): the input chunks are decoded on the GPU (destripe_zarr_store(device_decode=True)).
`device-decode-any`: the same with device_decode="any" (LZ4, split streams and bit shuffle go to the device too).
`device-decode-all`: the same with device_decode="full" (blosclz and zlib inside Blosc, and plain-zlib chunks, too).
`blosc-zlib`, `blosc-blosclz`, `plain-zlib` (Blosc only, N a multiple of 64): the INPUT store recoded like `lz4` below,
to Blosc frames with zlib (level 5) or blosclz inside (byte shuffle, 256 KiB blocks split in two streams; the greedy
blosclz encoder of tests/inflate_cases.py) or to the plain zlib compressor (level 1, one stream per 2 MiB chunk).
`lz4` (Blosc only, N a multiple of 64): the INPUT store is what numcodecs.Blosc() writes by default -- LZ4, byte
shuffle, 256 KiB blocks split into a low-byte and a high-byte stream (the test suite's LZ4 encoder,
tests/blosc_any_frames.py; every 64-plane block holds the same planes, as in the other variants); the output stays
Blosc-zstd.  The line then reports the input store's bytes and the chunks decoded on the device / host / filled.
`lz4-out` (Blosc only): the OUTPUT store (and the pyramid levels) is Blosc-LZ4 -- what numcodecs.Blosc() writes by default:
LZ4, clevel 5, byte shuffle, split streams -- written by the host LZ4 writer on the I/O threads, or with `device-codec` by
the device LZ4 encoder (csrc/dsx_lz4_enc.h; the same files either way).  The host writer's bytes reported for
comparison are then LZ4 frames too.
`read-back` (Blosc only): after the timed pass the written store is the input of one more pass with device_decode="any"
(into a Blosc-zstd store, device_codec="runs"); the line reports its seconds, read stage time and decode routes as "read_back".
`streaks`: the dual-band filter (destripe_zarr_store(streaks={"sigma": (64, 128), "route": "auto"})) instead of the stripe
filter ("auto" is the generic route until the march route's rate is on record, engine.AUTO_ROUTE); `streaks-generic` /
`streaks-march` name the route.  The picked planes are then held to destripe_streaks_planes of
the same route, bit for bit (no CPU oracle pass).
`ome-percentile`: both metadata options on -- every timed pass counts its filtered voxels on the device
(destripe_zarr_store(histogram=...)), takes the display window from the counts (display_window_from_histogram) and, with
a pyramid word (the output is then a group), writes .zgroup / .zattrs (write_ome_ngff_metadata), all inside the timed
seconds; the line reports the window and the voxels counted under "ome", and a count other than N * 2048 * 2048 fails the run.
`projections`: every timed pass collects the QC projections of the planes it writes (destripe_zarr_store(projections=
{"output": ...}); `projections-both`: of the planes it read as well), inside the timed seconds; the line reports the mode and
the planes added under "projections", and the rows of the picked planes are held to NumPy (a mismatch fails the run).
`digests`: every timed pass writes the digest manifests of its arrays (destripe_zarr_store(digests=True), and the
stand-alone pyramid words' compute_multiscale(digests=True)), inside the timed seconds; the written store is then read back
once with integrity.verify_store(device_decode=True) and once with device_decode=False, and the line reports both times,
the chunks checked and the bad ones under "digests" (any bad chunk fails the run).
`store-sha` (implied by `digests`): after the timed section every chunk file and .zarray of the output is read again and
hashed (the digest sidecars left out) and the line carries "store_sha256": equal between a run with `digests` and one
without.
`scale-FZ-FY-FX` (with a pyramid word): the pyramid's scale factor per axis, 1 or 2 each, e.g. `scale-1-2-2` for a volume
whose z step is coarser than its pixel (scale_factor of destripe_zarr_store / compute_multiscale); the default is 2-2-2.
`pyramid`: after the timed level-0 pass, compute_multiscale(n_levels=3) on the store is timed too (the two-pass route);
`fused-pyramid`: level 0 and levels 1-2 in one destripe_zarr_store call (pyramid_group / n_levels);
`pipelined-pyramid`: level 0 is timed as without a pyramid word, then compute_multiscale(pipelined=True, n_levels=3) with the
codec words given (device-decode only on a Blosc store) -- its line carries pyramid.LAST_PYRAMID as "pipelined".  All add level-0,
pyramid and total seconds, the levels' bytes on disk (with the host writer's frames of each level's first chunk row for
comparison) and a check of the first level-1 / level-2 planes against the NumPy oracle.
Every line reports the read / write stage times of the timed pass (I/O threads, summed per block), the bytes that
crossed the host link each way, and the link fraction those bytes make of the run (63 GB/s per direction)."""
import json, logging, os, shutil, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import synth, zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

logging.basicConfig(level=logging.INFO, stream=sys.stderr)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
codec = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "raw" else None  # None (raw chunks), "zlib" or "blosc" (Blosc-zstd)
device_codec = "runs" if "device-codec-runs" in sys.argv[3:] else "device-codec" in sys.argv[3:]
device_decode = ("full" if "device-decode-all" in sys.argv[3:] else
                 "any" if "device-decode-any" in sys.argv[3:] else "device-decode" in sys.argv[3:])
recode = ([w for w in ("lz4", "blosc-zlib", "blosc-blosclz", "plain-zlib") if w in sys.argv[3:]] + [None])[0]
lz4_input = recode is not None  # (any recoded input store)
two_pass, fused, pipelined = ("pyramid" in sys.argv[3:], "fused-pyramid" in sys.argv[3:], "pipelined-pyramid" in sys.argv[3:])
lz4_out, read_back = "lz4-out" in sys.argv[3:], "read-back" in sys.argv[3:]
streaks = ([{"sigma": (64.0, 128.0), "route": r} for w, r in (("streaks", "auto"), ("streaks-generic", "generic"),
                                                               ("streaks-march", "march")) if w in sys.argv[3:]] + [None])[0]
ome = "ome-percentile" in sys.argv[3:]
proj_keys = ("output", "input") if "projections-both" in sys.argv[3:] else ("output",) if "projections" in sys.argv[3:] else ()
digests = "digests" in sys.argv[3:]
scale = ([[int(f) for f in w.split("-")[1:]] for w in sys.argv[3:] if w.startswith("scale-")] + [[2, 2, 2]])[0]
if (lz4_out or read_back) and codec != "blosc":
    sys.exit("lz4-out / read-back: a Blosc store")
out_codec = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0} if lz4_out else codec
host_frame = dict(clevel=5, shuffle=True, cname="lz4") if lz4_out else dict(clevel=3, shuffle=True)
H = W = 2048
root = tempfile.mkdtemp(prefix="dsx_zarr_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    t0 = time.perf_counter()
    bank = synth.synthetic_bank(8, H, W)
    if lz4_input:
        if codec != "blosc" or n % 64:
            sys.exit(recode + ": a Blosc store of a multiple of 64 planes")
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import multiprocessing, zlib
        import blosc_any_frames as baf
        import inflate_cases as ic
        cname = {"lz4": "lz4", "blosc-zlib": "zlib", "blosc-blosclz": "blosclz"}.get(recode)
        src = MiniZarrArray.create(os.path.join(root, "in.zarr"), (1, 1, n, H, W), (1, 1, 64, 128, 128), np.uint16,
                                   compressor={"id": "blosc", "cname": cname, "clevel": 5, "shuffle": 1, "blocksize": 0}
                                   if cname else "zlib")
        stack = synth.synthetic_stack(64, H, W, bank=bank)
        yx = [(y, x) for y in range(H // 128) for x in range(W // 128)]
        raws = [np.ascontiguousarray(stack[:, 128 * y : 128 * y + 128, 128 * x : 128 * x + 128]).tobytes() for y, x in yx]
        with multiprocessing.Pool(16) as pool:  # (before anything touches the GPU)
            if recode == "lz4":
                frames = pool.starmap(baf.blosc_frame, [(r, 256 * 1024, baf.LZ4, baf.SHUFFLE, True) for r in raws])
            elif recode == "plain-zlib":
                frames = pool.starmap(zlib.compress, [(r, 1) for r in raws])
            else:
                inner = ic.ZLIB if recode == "blosc-zlib" else baf.BLOSCLZ
                frames = pool.starmap(ic.blosc_frame, [(r, 256 * 1024, inner, baf.SHUFFLE, True) for r in raws])
            pool.close()  # the workers leave by themselves: under rocprofv3, which handles SIGTERM in every child, the
            pool.join()   # terminate() of the with-block never saw them exit and the run hung before it reached the GPU
        for zb in range(n // 64):
            for (y, x), f in zip(yx, frames):
                p = src._chunk_path((0, 0, zb, y, x))
                os.makedirs(os.path.dirname(p), exist_ok=True)
                with open(p, "wb") as fh:
                    fh.write(f)
        del stack, raws
    else:
        src = MiniZarrArray.create(os.path.join(root, "in.zarr"), (1, 1, n, H, W), (1, 1, 64, 128, 128), np.uint16, compressor=codec)
        for z in range(0, n, 64):
            src[0, 0, z : z + 64] = synth.synthetic_stack(min(64, n - z), H, W, bank=bank)
    t_make = time.perf_counter() - t0
    res = {}
    group = os.path.join(root, "out.zarr")
    level0 = os.path.join(group, "0") if two_pass or fused or pipelined else group
    for name, kw in (("overlapped", {"pyramid_group": group, "n_levels": 3, "scale_factor": scale} if fused else {}),):
        for rep in range(2):  # second pass: plan + pinned buffers exist, page cache warm
            t0 = time.perf_counter()
            hist = np.zeros(65536, np.int64) if ome else None
            if proj_keys:
                from aind_smartspim_destripe_amd import projections as pj
                proj = {key: pj.VolumeProjections((n, H, W)) for key in proj_keys}
                kw = {**kw, "projections": proj}
            planes, dt = zd.destripe_zarr_store(os.path.join(root, "in.zarr"), level0, synth.CELLS_CONFIG,
                                          synth.NO_CELLS_CONFIG, None, prediction_chunksize=(64, H, W),
                                          output_chunks=(1, 1, 64, 128, 128), device=0, device_retile=True, io_threads=16, compressor=out_codec,
                                          device_codec=device_codec, device_decode=device_decode, streaks=streaks,
                                          **({"histogram": hist} if ome else {}), **({"digests": True} if digests else {}), **kw)
            if ome:
                window = zd.display_window_from_histogram(hist)
                if level0 != group:
                    zd.write_ome_ngff_metadata(group, MiniZarrArray.open(level0), "bench", 3, scale, [2.0, 1.8, 1.8],
                                               channel_names=["bench"], channel_colors=[zd.REFERENCE_CHANNEL_COLOR],
                                               channel_minmax=[(0, 65535)], channel_startend=[window])
            res[name] = {"planes": planes, "seconds": round(time.perf_counter() - t0, 3)}
    timing = dict(zd._BLOCKS["blocks"][1].timing)  # the timed (second) pass
    decode = {"decode_routes": zd.LAST_RUN.get("decode_routes")}
    if lz4_input:
        decode["input_store_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(src.path)
                                          for f in fs if not f.startswith("."))
        decode["input_ratio_to_raw"] = round(decode["input_store_bytes"] / (n * H * W * 2), 4)
    secs = res["overlapped"]["seconds"]
    ome_info = {}
    if ome:
        ome_info = {"ome": {"display_window": list(window), "histogram_voxels": int(hist.sum()),
                            "metadata_written": os.path.exists(os.path.join(group, ".zattrs"))}}
    pyr = {}
    if two_pass or fused or pipelined:
        pyramid_s = 0.0
        if pipelined:  # one pipelined device pass over the finished level 0 (compute_multiscale(pipelined=True))
            from aind_smartspim_destripe_amd import pyramid
            t0 = time.perf_counter()
            zd.compute_multiscale(level0, group, scale, 1, None, "bench", n_levels=3, compressor=out_codec, device=0,
                                  pipelined=True, device_codec=device_codec, io_threads=16,
                                  device_decode=device_decode if codec == "blosc" else False, **({"digests": True} if digests else {}))
            pyramid_s = time.perf_counter() - t0
            pyr["pipelined"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in pyramid.LAST_PYRAMID.items()}
        if two_pass:  # the route destripe_zarr takes by default: rank 0 reads level 0 back and writes the levels
            t0 = time.perf_counter()
            zd.compute_multiscale(level0, group, scale, 1, None, "bench", n_levels=3, compressor=out_codec, device=0,
                                  **({"digests": True} if digests else {}))
            pyramid_s = time.perf_counter() - t0
        pyr = {**pyr, "scale": scale, "route": "fused" if fused else ("pipelined" if pipelined else "two-pass"), "level0_s": round(secs, 3), "pyramid_s": round(pyramid_s, 3),
               "total_s": round(secs + pyramid_s, 3), "pyramid_download_bytes": int(timing["pyramid_download_bytes"])}
    up, down = int(timing["upload_bytes"]), int(timing["download_bytes"])
    link = {"upload_bytes": up, "download_bytes": down,
            "upload_GBps": round(up / secs / 1e9, 2), "download_GBps": round(down / secs / 1e9, 2),
            "frac": round(max(up, down) / secs / 63e9, 3)}
    out = MiniZarrArray.open(level0)
    chk = int(out[0, 0, 0].astype(np.uint64).sum())
    sizes = {}
    if codec == "blosc":  # bytes on disk; the host writer's frames of the first block's chunks for comparison
        from aind_smartspim_destripe_amd import mini_zarr
        written = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(level0)
                      for f in fs if not f.startswith("."))
        first = [out._chunk_path((0, 0, 0, y, x)) for y in range(H // 128) for x in range(W // 128)]
        got = sum(os.path.getsize(p) for p in first)
        host = sum(len(mini_zarr.blosc_encode(out._read_chunk((0, 0, 0, y, x)).tobytes(), 2, **host_frame))
                   for y in range(H // 128) for x in range(W // 128))
        sizes = {"bytes_written": written, "raw_bytes": n * H * W * 2, "ratio_to_raw": round(written / (n * H * W * 2), 4),
                 "first_block_bytes": got, "first_block_host_writer_bytes": host, "size_ratio_to_host_writer": round(got / host, 4)}
    if digests or "store-sha" in sys.argv[3:]:  # every chunk file and .zarray of the output, in path order
        import hashlib
        sha = hashlib.sha256()
        for rel in sorted(os.path.relpath(os.path.join(d, f), group) for d, _, fs in os.walk(group) for f in fs
                          if not f.startswith(".dsxdigest")):
            sha.update(rel.encode() + b"\0")
            with open(os.path.join(group, rel), "rb") as fh:
                sha.update(fh.read())
        sizes["store_sha256"] = sha.hexdigest()
    digest_info = {}
    if digests:  # read the written store back against its manifests: device decoders, then the host's
        from aind_smartspim_destripe_amd import integrity
        digest_info = {"digests": {"pass": zd.LAST_RUN.get("digests")}}
        for key, dd in (("verify_device_decode", True), ("verify_host_decode", False)):
            t0 = time.perf_counter()
            report = integrity.verify_store(group, device_decode=dd, io_threads=16, device=0)
            digest_info["digests"][key] = {"seconds": round(time.perf_counter() - t0, 3), "arrays": report["arrays"],
                                           "chunks": report["chunks"], "bad": [list(b) for b in report["bad"][:8]]}
    if read_back:  # the written store as the input of a pass that decodes it on the device
        for rep in range(2):  # (second pass: the staging buffers of this geometry exist)
            t0 = time.perf_counter()
            zd.destripe_zarr_store(level0, os.path.join(root, "back.zarr"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, None,
                                   prediction_chunksize=(64, H, W), output_chunks=(1, 1, 64, 128, 128), device=0,
                                   device_retile=True, io_threads=16, compressor="blosc", device_codec="runs", device_decode="any")
        sizes["read_back"] = {"seconds": round(time.perf_counter() - t0, 3),
                              "read_s": round(zd._BLOCKS["blocks"][1].timing["read_s"], 3),
                              "decode_routes": zd.LAST_RUN.get("decode_routes")}
        shutil.rmtree(os.path.join(root, "back.zarr"), ignore_errors=True)
    if pyr:
        from oracle import format_oracle as fo
        want = fo.pyramid(out[0, 0, 0:8], 3, scale)
        pyr["levels"], pyr["verified"] = {}, True
        for lvl in (1, 2):
            arr = MiniZarrArray.open(os.path.join(group, str(lvl)))
            pyr["verified"] = pyr["verified"] and bool(np.array_equal(arr[0, 0, 0 : want[lvl].shape[0]], want[lvl]))
            info = {"shape": list(arr.shape), "chunks": list(arr.chunks),
                    "bytes_written": sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(arr.path)
                                         for f in fs if not f.startswith("."))}
            if codec == "blosc":  # the level's first chunk row: bytes on disk against the host writer's frames
                idx = [(0, 0, 0, y, x) for y in range(-(-arr.shape[3] // arr.chunks[3])) for x in range(-(-arr.shape[4] // arr.chunks[4]))]
                info["first_row_bytes"] = sum(os.path.getsize(arr._chunk_path(i)) for i in idx)
                info["first_row_host_writer_bytes"] = sum(len(mini_zarr.blosc_encode(arr._read_chunk(i).tobytes(), 2, **host_frame)) for i in idx)
                info["size_ratio_to_host_writer"] = round(info["first_row_bytes"] / info["first_row_host_writer_bytes"], 4)
            pyr["levels"][str(lvl)] = info
    v = res["overlapped"]["planes"] / res["overlapped"]["seconds"]
    # ---- verification (tests/test_zarr_chunk_map.py::test_chunk_map_at_production_geometry_against_the_oracle holds the
    # same statement on a 192-plane store): one plane of every stream part of the first, a middle and the last block --
    # bit-identical to the same plane filtered alone (one launch chain, one stream); the first block's picks and planes
    # 0 / 1 also against the CPU oracle (uint16 truncation: one count; see parity_util.u16_plane_against_oracle)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from parity_util import stream_part_picks, u16_plane_against_oracle
    from aind_smartspim_destripe_amd import filtering as fl
    nblk = (n + 63) // 64
    blocks = sorted({0, nblk // 2, nblk - 1})
    verified, checked, oracle_checked = True, [], []
    if ome and int(hist.sum()) != n * H * W:
        verified = False
        print("histogram counted", int(hist.sum()), "voxels of", n * H * W, file=sys.stderr)
    proj_info = {}
    if proj_keys:
        proj_info = {"projections": {"mode": zd.LAST_RUN["projections"], "planes": zd.LAST_RUN["projection_planes"]}}
        verified = verified and all(p.added.all() for p in proj.values())
    for b in blocks:
        z0, z1 = 64 * b, min(64 * b + 64, n)
        for z in stream_part_picks(64, z0, z1):
            plane_in = src[0, 0, z]
            got = out[0, 0, z]
            for key, plane in (("output", got), ("input", plane_in)):
                if key in proj_keys:
                    want = pj.project_volume(plane[None])
                    if not all(np.array_equal(proj[key].arrays[k][z], want[k][0]) for k in ("max_y", "sum_y", "max_x", "sum_x")):
                        verified = False
                        print("projection mismatch", key, z, file=sys.stderr)
            if streaks is not None:
                alone = fl.destripe_streaks_planes(plane_in[None], streaks["sigma"], route=zd.LAST_RUN["streaks_route"],
                                                   out_dtype=np.uint16, max_batch=1)[0]
            else:
                alone = fl.destripe_planes(plane_in[None], "t", synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, 2500,
                                           out_dtype=np.uint16, max_batch=1)[0]
            if not np.array_equal(alone, got):
                verified = False
            checked.append(int(z))
            if b == 0 and streaks is None:
                try:
                    u16_plane_against_oracle(got, plane_in, "t", None, ("bench_zarr", z))
                    oracle_checked.append(int(z))
                except AssertionError as e:
                    verified = False
                    print("oracle mismatch", e, file=sys.stderr)
    label = (codec or "raw") + (", {} input".format("LZ4" if recode == "lz4" else recode) if lz4_input else "") + (", LZ4 output" if lz4_out else "") + (", encoded on the device" + (" with run matches" if device_codec == "runs" else "") if device_codec else "") + (", decoded on the device" + (" ({})".format(device_decode) if isinstance(device_decode, str) else "") if device_decode else "")
    label += ", dual-band filter ({} route)".format(zd.LAST_RUN["streaks_route"]) if streaks is not None else ""
    label += ", pyramid fused" if fused else ""  # (a stand-alone pyramid, slab or pipelined, is not part of the metric)
    print(json.dumps({"metric": "2048x2048 uint16 slices/s, Zarr store to Zarr store ({} chunks, tmpfs)".format(label), "value": round(v, 1),
                      "planes": n, "seconds": res["overlapped"]["seconds"], "store_make_s": round(t_make, 1),
                      "roofline": {"bound": "host link", "peak_planes_per_s": 3750, "frac": round(v / 3750.0, 3)},
                      "read_s": round(timing["read_s"], 3), "write_s": round(timing["write_s"], 3), "host_link": link,
                      "plane0_checksum": chk, "verified": verified,
                      "filter": zd.LAST_RUN.get("filter"), "streaks_route": zd.LAST_RUN.get("streaks_route"), **decode, **sizes, **ome_info, **proj_info, **digest_info, **({"pyramid": pyr} if pyr else {}),
                      "verification": {"planes_bit_identical_to_single_plane_runs": checked,
                                       "planes_against_the_cpu_oracle": oracle_checked, "blocks": blocks}}))
    if digests and any(v["bad"] for k, v in digest_info["digests"].items() if k != "pass"):
        sys.exit(3)
    if not verified or not pyr.get("verified", True):
        sys.exit(3)
finally:
    shutil.rmtree(root, ignore_errors=True)
