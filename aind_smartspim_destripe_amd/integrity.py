"""Reading a digest manifest back: fresh per-chunk digests of a store, and their comparison with what the writers
recorded (``csrc/dsx_digest.h``; the manifest is ``mini_zarr.DIGEST_JSON`` / ``DIGEST_BIN``).

Neither the Blosc frames nor the zstd frames of a store carry a checksum, and the input of a pass is deleted once the
destriped store exists.  :func:`verify_store` is what can be run over a store after a pass, after a copy, or a year
later, to say "these are the voxels the filter produced": every chunk is read and decoded again -- by the host decoders
(libzstd / liblz4 / zlib: the check that is independent of this project's code) or by the device decoders, which take
only compressed bytes across the host link -- and digested where it lies, by ``k_brick_digest_u16`` on the decoded
bricks or, with ``device=None``, by the host build, so that an archive can be checked on a machine without a GPU.

The digest is not cryptographic.  With ``device_decode`` a store is checked with this project's own decoders;
``device_decode=False`` is the independent check.
"""

import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import engine as engine_mod
from .mini_zarr import MiniZarrArray

REASONS = ("digest", "undecodable", "unrecorded", "no manifest", "bad manifest")
_BLOCK_BYTES = 256 << 20  # decoded voxels of one block of chunk rows (at least one row)


def _chunk_rows(arr):
    """``(grid, rows per block)`` of the chunk grid of ``arr`` (``ValueError`` for what the digest does not cover)."""
    from .mini_zarr import digest_grid_of

    grid = digest_grid_of(arr.shape, arr.chunks, arr.dtype)
    row_bytes = grid[1] * grid[2] * int(np.prod(arr.chunks[-3:])) * 2
    return grid, max(1, min(grid[0], _BLOCK_BYTES // row_bytes))


def _block_valid(arr, r0, rows):
    """Valid voxels that chunk rows ``[r0, r0 + rows)`` cover along each axis from the block's chunk-aligned origin."""
    Z, H, W = arr.shape[-3:]
    return (min(rows * arr.chunks[-3], Z - r0 * arr.chunks[-3]), H, W)


def _read_one(arr, idx, out_flat):
    """Chunk ``idx`` decoded by the host into ``out_flat``; returns the decoder's error text, or ``None``."""
    try:
        arr.read_chunk_into(idx, out_flat)
    except Exception as e:  # whatever a decoder says of a damaged file: the chunk is named, the pass goes on
        out_flat[...] = 0
        return "{}: {}".format(type(e).__name__, e)
    return None


def _read_singly(arr, idx, stage, pool):
    """Every chunk of a block on its own (a batched read raised): ``{position in the block: error text}``."""
    errs = list(pool.map(lambda t: _read_one(arr, t[1], stage[t[0]]), enumerate(idx)))
    return {i: e for i, e in enumerate(errs) if e is not None}


def _digest_host(arr, io_threads, errors):
    grid, _ = _chunk_rows(arr)
    lead = (0,) * (arr.ndim - 3)
    c = arr.chunks[-3:]
    brick = int(np.prod(c))
    out = np.zeros(int(np.prod(grid)), engine_mod.DIGEST_DTYPE)

    def one(t):
        n, g = t
        buf = np.empty(brick, np.uint16)
        err = _read_one(arr, lead + g, buf)
        if err is None:
            out[n] = engine_mod.brick_digest_ref(buf, (1, 1, 1), c, arr.digest_extents(g))[0]
        return n, err

    with ThreadPoolExecutor(max_workers=io_threads) as pool:
        for n, err in pool.map(one, enumerate(itertools.product(*[range(g) for g in grid]))):
            if err is not None:
                errors.append((n, err))
    return out


def _digest_device(arr, decode_mode, io_threads, device, errors):
    from . import filtering
    from .zarr_destriper import ZDEC_MODES, bad_stream_message, device_decode_input_ok

    if decode_mode is not None and not device_decode_input_ok(arr, decode_mode):
        decode_mode = None  # (raw chunks, or a codec the device does not read: the host decodes, the device digests)
    eng = next((e[0] for k, e in filtering._ENGINES.items() if k[0] == device), None)  # the process's engine, if any
    own = eng is None
    if own:
        eng = engine_mod.DestripeEngine(device)
    grid, rows = _chunk_rows(arr)
    lead = (0,) * (arr.ndim - 3)
    c = arr.chunks[-3:]
    brick = int(np.prod(c))
    per_row = grid[1] * grid[2]
    n_max = rows * per_row
    C, U = engine_mod.STREAM_COMPUTE, engine_mod.STREAM_UPLOAD
    out = np.zeros(int(np.prod(grid)), engine_mod.DIGEST_DTYPE)
    bufs = []

    def alloc(kind, nbytes):
        bufs.append(eng.alloc(nbytes) if kind == "d" else eng.alloc_host(nbytes))
        return bufs[-1]

    try:
        d_bricks, d_rec = alloc("d", n_max * brick * 2), alloc("d", n_max * engine_mod.DIGEST_DTYPE.itemsize)
        h_rec = alloc("h", n_max * engine_mod.DIGEST_DTYPE.itemsize).array((n_max,), engine_mod.DIGEST_DTYPE)
        stage = alloc("h", n_max * brick * 2).array((n_max, brick), np.uint16)
        if decode_mode is not None:
            cap = n_max * (brick * 2 + 16)
            n_tasks = n_max * engine_mod.frame_tasks_per_chunk(brick * 2)
            packed = alloc("h", cap).array((cap,), np.uint8)
            tasks = alloc("h", n_tasks * engine_mod.TASK_DTYPE.itemsize).array((n_tasks,), engine_mod.TASK_DTYPE)
            status = alloc("h", 4 * n_tasks).array((n_tasks,), np.int32)
            d_packed, d_tasks, d_status = alloc("d", cap), alloc("d", n_tasks * engine_mod.TASK_DTYPE.itemsize), alloc("d", 4 * n_tasks)
            zlib_chunks = arr.compressor[0] == "zlib"
        with ThreadPoolExecutor(max_workers=io_threads) as pool:
            for r0 in range(0, grid[0], rows):
                nr = min(rows, grid[0] - r0)
                idx = [lead + (r0 + g[0], g[1], g[2]) for g in itertools.product(range(nr), range(grid[1]), range(grid[2]))]
                n = len(idx)
                paths = [arr._chunk_path(i) for i in idx]
                bad, nt = {}, 0
                try:
                    if decode_mode is not None:
                        pb, nt = eng.io_read_frames(paths, brick * 2, packed, tasks, threads=io_threads,
                                                    fill_value=int(arr.fill_value), mode=ZDEC_MODES[decode_mode],
                                                    zlib_chunks=zlib_chunks)  # fmt: skip
                    else:
                        eng.io_read_chunks(paths, [stage[i] for i in range(n)], threads=io_threads, codec=arr.codec,
                                           fill_value=int(arr.fill_value))  # fmt: skip
                except Exception:  # a damaged file stops the batched read at the first: name every one of the block
                    bad, nt = _read_singly(arr, idx, stage, pool), -1
                if nt >= 0 and decode_mode is not None:
                    if pb:
                        eng.copy_h2d_async(d_packed, packed[:pb], U)
                    if nt:
                        eng.copy_h2d_async(d_tasks, tasks[:nt], U)
                    eng.stream_wait(C, U)
                    eng.blosc_decode_device(d_packed, pb, d_tasks, nt, d_bricks, d_status, out_bytes=n * brick * 2)
                    if nt:
                        eng.copy_d2h_async(status[:nt], d_status, C)
                else:
                    eng.copy_h2d_async(d_bricks, stage[:n], U)
                    eng.stream_wait(C, U)
                eng.brick_digest(d_bricks, (nr, grid[1], grid[2]), c, _block_valid(arr, r0, nr), d_rec, stream=C)
                eng.copy_d2h_async(h_rec[:n], d_rec, C)
                eng.stream_sync(C)  # (the staging buffers are reused by the next block)
                eng.stream_sync(U)
                first = r0 * per_row
                out[first : first + n] = h_rec[:n]
                if nt > 0:
                    for t in np.flatnonzero(status[:nt]):
                        k = int(tasks["chunk"][t])
                        bad.setdefault(k, bad_stream_message(int(tasks["kind"][t]), paths[k], int(status[t]), zlib_chunks))
                for k, msg in sorted(bad.items()):
                    out[first + k] = (0, 0, 0)
                    errors.append((first + k, msg))
    finally:
        for b in bufs:
            b.free()
        if own:
            eng.close()
    return out


def digest_store(array_path, device_decode=False, io_threads=None, device=0, errors=None):
    """Fresh records of every chunk of the array at ``array_path``: ``engine.DIGEST_DTYPE[g0 * g1 * g2]`` in C order of
    the chunk grid, what a manifest of the array holds when the store is intact.  A missing chunk file has the record of
    ``fill_value`` everywhere.

    The chunk files go through ``io_threads`` I/O threads and are decoded by the host (``device_decode=False``) or on
    the device (``True`` / ``"any"`` / ``"full"`` as in ``destripe_zarr_store``; an array the device decoders do not
    read is decoded by the host); the digests are computed by the kernel on the decoded bricks.  With ``device=None``
    everything runs on the host build and no GPU is needed.  ``errors``: a list that receives ``(chunk index, message)``
    for every chunk that does not decode (its record is zero); without one the first such chunk is a ``ValueError``."""
    from .zarr_destriper import default_io_threads, device_decode_mode

    arr = array_path if isinstance(array_path, MiniZarrArray) else MiniZarrArray.open(str(array_path))
    decode_mode = device_decode_mode(device_decode)
    io_threads = int(io_threads) if io_threads else default_io_threads()
    errs = []
    if device is None:
        rec = _digest_host(arr, io_threads, errs)
    else:
        rec = _digest_device(arr, decode_mode, io_threads, device, errs)
    errs.sort()
    if errors is None and errs:
        raise ValueError("chunk {} of {} does not decode: {}".format(errs[0][0], arr.path, errs[0][1]))
    if errors is not None:
        errors.extend(errs)
    return rec


def _arrays_of(path):
    """The arrays under ``path``: the array itself, or the numbered children of a group, in numeric order."""
    path = str(path)
    if os.path.exists(os.path.join(path, ".zarray")):
        return [path]
    kids = sorted((d for d in os.listdir(path) if d.isdigit() and os.path.exists(os.path.join(path, d, ".zarray"))), key=int)
    if not kids:
        raise ValueError("{} is neither a Zarr array nor a group of numbered arrays".format(path))
    return [os.path.join(path, d) for d in kids]


def verify_store(path, device_decode=False, io_threads=None, device=0):
    """Compare every chunk of an array, or of every numbered array of a group (the levels of a tile), with the array's
    digest manifest.  Returns ``{"arrays": n, "chunks": chunks checked, "bad": [(array path, chunk index, reason)],
    "detail": {(array path, chunk index): text}}``; ``reason`` is one of

    * ``"digest"``: the chunk decodes, to other voxels than were recorded;
    * ``"undecodable"``: the chunk does not decode (``detail`` has the device task's status or the host decoder's error);
    * ``"unrecorded"``: the manifest has no record of the chunk (``count == 0``);
    * ``"no manifest"``: the array keeps none (chunk index ``None``);
    * ``"bad manifest"``: the array's ``.dsxdigest.bin`` cannot be read or does not hold one record per chunk -- a torn
      or truncated sidecar (chunk index ``None``, ``detail`` has the error); the array's chunks are not compared.

    Never stops at the first bad chunk, nor at the first bad array.  Every numbered child of a group is held to having a
    manifest: a level left in the folder by an earlier run that wrote more levels is reported as ``"no manifest"`` (and
    fails ``destripe_zarr(verify=True)``) until it is removed.  Arguments as :func:`digest_store`."""
    report = {"arrays": 0, "chunks": 0, "bad": [], "detail": {}}
    for p in _arrays_of(path):
        arr = MiniZarrArray.open(p)
        report["arrays"] += 1
        if arr.digest_grid is None:
            report["bad"].append((p, None, "no manifest"))
            continue
        try:
            want = arr.digest_records()
        except (ValueError, OSError) as e:
            report["bad"].append((p, None, "bad manifest"))
            report["detail"][(p, None)] = str(e)
            continue
        errs = []
        got = digest_store(arr, device_decode=device_decode, io_threads=io_threads, device=device, errors=errs)
        report["chunks"] += want.size
        undecodable = dict(errs)
        for n in range(want.size):
            if n in undecodable:
                report["bad"].append((p, n, "undecodable"))
                report["detail"][(p, n)] = undecodable[n]
            elif want["count"][n] == 0:
                report["bad"].append((p, n, "unrecorded"))
            elif want[n] != got[n]:
                report["bad"].append((p, n, "digest"))
                report["detail"][(p, n)] = "recorded {} computed {}".format(tuple(int(x) for x in want[n]), tuple(int(x) for x in got[n]))
    return report


def format_bad(report, limit=20):
    """The bad chunks of a report as text (for an exception): at most ``limit`` of them, and their number."""
    lines = ["{} chunk {}: {}".format(p, n, reason) for p, n, reason in report["bad"][:limit]]
    more = len(report["bad"]) - len(lines)
    return "; ".join(lines) + ("; and {} more".format(more) if more > 0 else "")
