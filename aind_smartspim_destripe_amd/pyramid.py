"""Multiscale pyramid of the destriped volume on the GPU.

Mirrors ``compute_pyramid`` (``/root/reference/code/aind_smartspim_destripe/zarr_destriper.py:365-407``) and the
level loop of ``compute_multiscale`` (``:677-794``): ``xarray_multiscale.multiscale`` with the
``windowed_mean`` reducer, ``scale_factors`` 2 per spatial axis and ``preserve_dtype=True`` -- every level
is the 2 x 2 x 2 windowed mean of the previous one, truncated back to uint16 -- without the dask
``LocalCluster`` (``:689-697``): one HIP kernel per level (``dsx_downsample2_u16``), the volume stays in HBM
between levels.  No CPU fallback.

The window is a parameter as in the reference (``scale_axis`` / ``scale_factor``): 1 or 2 per spatial axis, not all 1
(:func:`_check_scale`), so an anisotropic volume can reduce only its fine axes, e.g. ``(1, 2, 2)``.  ``(2, 2, 2)`` runs
the kernels named here; any other scale runs ``k_pyramid_step<FZ, FY, FX>`` once per level on every route.
"""

import itertools
import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import engine as _engine
from .distributed import z_shard
from .mini_zarr import MiniZarrArray


def _check_scale(scale_axis):
    """``(fz, fy, fx)`` of ``scale_axis`` (``compute_pyramid``) / ``(1, 1) + scale_factor`` (``compute_multiscale``):
    1 or 2 per spatial axis, not all 1, behind unit leading axes; ``ValueError`` otherwise."""
    try:
        scale = list(scale_axis)
        lead_ok = len(scale) >= 3 and all(s == 1 for s in scale[:-3])
    except TypeError:
        scale, lead_ok = [], False
    if not lead_ok:
        raise ValueError("only scale factors (.., fz, fy, fx) behind unit leading axes are implemented, not {!r}"
                         .format(scale_axis))  # fmt: skip
    return _engine.pyramid_scale(scale[-3:])


def check_scale_factor(scale_factor):
    """``(fz, fy, fx)`` of a ``scale_factor`` of ``compute_multiscale``: three factors, :func:`_check_scale`'s rules."""
    try:
        axes = (1, 1) + tuple(scale_factor)
    except TypeError:
        axes = ()
    if len(axes) != 5:
        raise ValueError("only scale factors (fz, fy, fx) are implemented, not {!r}".format(scale_factor))
    return _check_scale(axes)


def _window(scale, level):
    """Level-0 planes under one plane of level ``level``."""
    return int(scale[0]) ** int(level)


# ---- the pyramid fused into the destripe pass (zarr_destriper.destripe_zarr_store(pyramid_group=...)) -----------------
# One level of the plan: its index, its [Z, Y, X] shape and its chunk shape (clamped to the shape).
FusedLevel = namedtuple("FusedLevel", "level shape chunks")
# One level's share of one z block: chunk row, first plane inside the row, planes, whether the block is the first to
# touch the row (the row must be zeroed) and whether the row leaves after this block.
BlockShare = namedtuple("BlockShare", "level row offset planes first flush")


def fused_levels(zyx, chunks, n_levels, scale=(2, 2, 2)):
    """Levels ``1 .. n_levels - 1`` as :func:`write_pyramid_levels` writes them: shape ``n // f`` of the previous
    level per axis (``f`` of ``scale``), chunks ``min(c, n)``, stopping at a source level with an axis shorter than its
    factor."""
    levels, cur = [], tuple(int(n) for n in zyx)
    for i in range(1, int(n_levels)):
        if any(n < f for n, f in zip(cur, scale)):
            break
        cur = tuple(n // f for n, f in zip(cur, scale))
        levels.append(FusedLevel(i, cur, tuple(min(int(c), n) for c, n in zip(tuple(chunks)[-3:], cur))))
    return levels


def fused_z_chunk(z_chunk, levels, scale=(2, 2, 2)):
    """z alignment of the rank shards: one chunk row of the deepest level, in level-0 planes
    (``cz << (levels written - 1)``; ``cz * fz ** levels`` in general, so the plain output z chunk when z is not
    reduced), so that every chunk of every level is written by exactly one rank."""
    return int(z_chunk) * _window(scale, len(levels))


def fused_z_range(n_slices, world_size, rank, z_chunk, levels, scale=(2, 2, 2)):
    return z_shard(n_slices, world_size, rank, z_chunk=fused_z_chunk(z_chunk, levels, scale))


def fused_check_blocks(levels, block_z, scale=(2, 2, 2)):
    """``ValueError`` unless z blocks of ``block_z`` planes hold whole windows of every level and fill whole chunk rows."""
    if levels and block_z % _window(scale, len(levels)):
        raise ValueError("fused_pyramid needs z blocks of a multiple of {} planes ({} x {} x {} windows of {} levels), "
                         "not {}".format(_window(scale, len(levels)), *scale, len(levels), block_z))  # fmt: skip
    for lv in levels:
        row = lv.chunks[0] * _window(scale, lv.level)
        if lv.shape[0] > lv.chunks[0] and row % block_z:
            raise ValueError("fused_pyramid needs z blocks that fill whole chunk rows of every level: {} planes do not "
                             "divide the {} of a level-{} chunk row".format(block_z, row, lv.level))  # fmt: skip


def fused_schedule(levels, z_start, z_stop, block_z, scale=(2, 2, 2)):
    """What every z block of ``[z_start, z_stop)`` (a :func:`fused_z_range`) gives to every level:
    ``[((z0, z1), [BlockShare per level])]``.  A chunk row leaves (``flush``) with the block that completes it, or with
    the last block of the range when it holds anything."""
    out, filled = [], [0] * len(levels)
    starts = list(range(z_start, z_stop, block_z))
    for z0 in starts:
        z1, shares = min(z0 + block_z, z_stop), []
        for i, lv in enumerate(levels):
            w = _window(scale, lv.level)
            p0, n, cz = z0 // w, (min(z0 + block_z, z_stop) - z0) // w, lv.chunks[0]
            row, off = divmod(p0, cz)
            if n and off + n > cz:
                raise ValueError("a z block straddles a level-{} chunk row (fused_check_blocks)".format(lv.level))
            filled[i] += n
            done = filled[i] > 0 and ((p0 + n) % cz == 0 or z0 == starts[-1])
            shares.append(BlockShare(lv.level, row, off, n, off == 0, done))
            if done:
                filled[i] = 0
        out.append(((z0, z1), shares))
    return out


def pipelined_block_z(src_cz, levels, scale=(2, 2, 2)):
    """z block of the pipelined stand-alone pyramid: the smallest multiple of the source z chunk ``src_cz`` (blocks are
    whole source chunks) that :func:`fused_check_blocks` accepts.  The first condition there holds from
    ``lcm(src_cz, 2^levels) <= src_cz << levels`` on (``fz ** levels`` for 2 in general), and a block the chunk rows
    refuse has no multiple they accept, so the search is bounded; ``ValueError`` when it finds nothing."""
    src_cz = int(src_cz)
    if src_cz <= 0:
        raise ValueError("the source z chunk must be positive, not {}".format(src_cz))
    for m in range(1, _window(scale, len(levels)) + 1):
        try:
            fused_check_blocks(levels, m * src_cz, scale)
        except ValueError:
            continue
        return m * src_cz
    raise ValueError("pipelined pyramid: no z block of whole source chunks ({} planes each) holds whole {} x {} x {} windows "
                     "of {} levels and fills whole chunk rows of every level (z chunks {})".format(
                         src_cz, *scale, len(levels), [lv.chunks[0] for lv in levels]))  # fmt: skip


def compute_pyramid(data, n_lvls, scale_axis, chunks="auto", device=0, engine=None):
    """``zarr_destriper.py:365-407``: ``[level 0 (the input), level 1, ...]``, ``n_lvls`` entries.

    ``data``: uint16 with the spatial axes last (``[Z, Y, X]`` up to ``[1, 1, Z, Y, X]``; leading axes must be
    singletons); ``chunks`` is accepted for signature parity and ignored (dense arrays come back).

    ``scale_axis``: :func:`_check_scale`'s factors with ``fy == fx`` -- ``(2, 2, 2)``, ``(1, 2, 2)``, ``(2, 1, 1)``: the
    pixel of a plane is square, so this in-memory entry point reduces y and x together or not at all, and it goes on
    refusing a window such as ``(2, 2, 1)`` as it always did (``ValueError`` before a device is touched).  The store
    routes (:func:`write_pyramid_levels`, the fused pass) take every scale of :func:`_check_scale`.
    """
    scale = _check_scale(scale_axis)
    if scale[1] != scale[2]:
        raise ValueError("only scale factors that reduce y and x alike (fy == fx) are implemented by compute_pyramid, "
                         "not {!r}".format(scale_axis))  # fmt: skip
    vol = np.asarray(data)
    if vol.dtype != np.uint16:
        raise ValueError("the pyramid kernel takes uint16 volumes (what the destriped Zarr stores)")
    lead = vol.shape[:-3]
    if any(n != 1 for n in lead):
        raise ValueError("leading (t, c) axes must be singletons")
    zyx = tuple(vol.shape[-3:])
    eng = engine or _engine.DestripeEngine(device)
    levels = [vol]
    bufs = []
    try:
        d_prev = eng.alloc(max(vol.nbytes, 16))
        bufs.append(d_prev)
        d_prev.upload(np.ascontiguousarray(vol))
        for _ in range(1, int(n_lvls)):
            if any(n < f for n, f in zip(zyx, scale)):
                break
            nxt = tuple(n // f for n, f in zip(zyx, scale))
            d_next = eng.alloc(max(int(np.prod(nxt)) * 2, 16))
            bufs.append(d_next)
            eng.downsample2(d_prev, d_next, zyx, scale)
            levels.append(d_next.download(nxt, np.uint16).reshape(lead + nxt))
            d_prev, zyx = d_next, nxt
    finally:
        for b in bufs:
            b.free()
        if engine is None:
            eng.close()
    return levels


def write_pyramid_levels(level0_path, group_path, scale_factor=(2, 2, 2), n_levels=3, chunks=(1, 1, 64, 128, 128),
                       compressor="blosc", device=0, slab_planes=None, pipelined=False, device_codec=False,
                       device_decode=False, io_threads=None, digests=False):  # fmt: skip
    """Level loop of ``compute_multiscale`` (``zarr_destriper.py:746-782``) over Zarr-v2 directory stores
    (``zarr_destriper.compute_multiscale`` is the entry point with the reference's signature and calls this):
    writes ``<group_path>/<i>`` for ``i = 1 .. n_levels - 1`` (uint16, ``"/"`` separator), every level from the
    previous one.  The OME-NGFF metadata (``:728-742``) is written by the caller
    (``zarr_destriper.compute_multiscale(ome_metadata=True)``), not here.  Returns the written arrays' shapes.

    The volume is streamed in z-slabs (a 34 GB channel does not fit one allocation, nor host RAM twice):
    a slab of ``2 * output z-chunk`` source planes is read, reduced by one ``dsx_downsample2_u16`` launch
    and written as whole output chunks; the 2 x 2 x 2 windows never straddle a slab because slabs start
    at even planes.  ``scale_factor`` ``(fz, fy, fx)``, 1 or 2 each and not all 1, is the window of every level on
    both routes (a slab is then ``fz * output z-chunk`` planes and level ``i`` is ``previous // factor`` per axis).

    ``pipelined=True``: the same arrays, chunk files and voxels from ONE software-pipelined pass over level 0
    (:class:`_PipelinedPyramid`): level 0 is read block by block on ``io_threads`` native threads straight into pinned
    staging, every level is computed from the block where it lies in chunk order (``dsx_pyramid_bricks_u16``) and the
    finished chunk rows leave through the I/O threads; no level is read back.  ``device_decode`` / ``device_codec``
    (``False``, ``True``, ``"any"``, ``"full"`` / ``"runs"``: ``zarr_destriper.device_decode_mode`` / ``device_codec_mode``) move the
    Blosc decode of level 0 and the Blosc-zstd encode of the levels to the GPU; they need a Blosc uint16 input / a
    Blosc-zstd uint16 output with byte shuffle, and ``pipelined``.  ``slab_planes`` is ignored then.
    :data:`LAST_PYRAMID` holds what the call did.

    ``digests``: every level is created with a digest manifest (``MiniZarrArray.create(digests=True)``).  The slab route
    fills it through the array's own writes (the host build); the pipelined route digests every finished chunk row on
    the device where it lies (``dsx_brick_digest_u16_device``, behind the pyramid kernel and before the encoder) and
    the writer of the row stores its records.  Off: no launch, allocation or file differs.
    """
    scale = check_scale_factor(scale_factor)
    fz, fy, fx = scale
    if pipelined:
        return _write_pipelined(level0_path, group_path, n_levels, chunks, compressor, device, device_codec, device_decode,
                                io_threads, scale, bool(digests))  # fmt: skip
    if device_codec is not False or device_decode is not False:
        raise ValueError("device_codec / device_decode need pipelined=True: the slab route of write_pyramid_levels has no "
                         "device codecs")  # fmt: skip
    t_start = time.perf_counter()
    eng = _engine.DestripeEngine(device)
    shapes = []
    try:
        src_path = level0_path
        for i in range(1, int(n_levels)):
            src = MiniZarrArray.open(src_path)
            if src.dtype != np.uint16 or any(n != 1 for n in src.shape[:-3]):
                raise ValueError("the pyramid kernel takes uint16 volumes with singleton leading axes")
            Z, Y, X = src.shape[-3:]
            if Z < fz or Y < fy or X < fx:
                break
            out_zyx = (Z // fz, Y // fy, X // fx)
            lead = src.shape[:-3]
            out_shape = lead + out_zyx
            ck = tuple(min(c, n) for c, n in zip(tuple(chunks)[-len(out_shape):], out_shape))
            dst = MiniZarrArray.create(os.path.join(group_path, str(i)), out_shape, ck, np.uint16,
                                       compressor=compressor, dimension_separator="/", digests=bool(digests))  # fmt: skip
            slab = int(slab_planes) if slab_planes else fz * ck[-3]
            slab += -slab % fz
            d_src = eng.alloc(slab * Y * X * 2)
            d_dst = eng.alloc(max((slab // fz) * out_zyx[1] * out_zyx[2] * 2, 16))
            try:
                lead_idx = (0,) * len(lead)
                for z in range(0, fz * out_zyx[0], slab):
                    n = min(slab, fz * out_zyx[0] - z)  # whole windows: an odd trailing plane is cropped
                    d_src.upload(src[lead_idx + (slice(z, z + n),)])
                    eng.downsample2(d_src, d_dst, (n, Y, X), scale)
                    out = d_dst.download((n // fz,) + out_zyx[1:], np.uint16)
                    dst[lead_idx + (slice(z // fz, z // fz + n // fz),)] = out
            finally:
                d_src.free()
                d_dst.free()
            shapes.append(out_shape)
            src_path = os.path.join(group_path, str(i))
    finally:
        eng.close()
    LAST_PYRAMID.clear()
    LAST_PYRAMID.update(route="slabs", block_z=None, levels=list(range(1, len(shapes) + 1)), decode_routes=None, read_s=None,
                        scale=scale, write_s=None, upload_bytes=None, download_bytes=None, seconds=time.perf_counter() - t_start,
                        digests=bool(digests))  # fmt: skip
    return shapes


# ---- the stand-alone pyramid in one pipelined pass (write_pyramid_levels(pipelined=True)) ----------------------------
# What the last write_pyramid_levels call of this process did: route ("pipelined" / "slabs"), block_z, levels,
# scale ((fz, fy, fx)), decode_routes ({"device", "host", "fill"}: level-0 chunks by where they were decoded), read_s / write_s (time inside
# the I/O stages), upload_bytes / download_bytes over the host link, seconds, digests (were manifests written).  The slab
# route fills route, levels, seconds, digests.
LAST_PYRAMID = {}


class _PipelinedPyramid:
    """One pass over a finished level 0 that writes every pyramid level, software-pipelined like the level-0 pass
    (``zarr_destriper._DeviceBlocks``: three streams, two sets of buffers, the two rules of its docstring) but without a
    filter and without a level-0 output.

    A block is ``block_z`` planes = whole source chunk rows (:func:`pipelined_block_z`), so it starts on a source chunk
    boundary and goes to the device as it lies in the store.  While block ``b`` is reduced on the compute stream
    (``dsx_pyramid_bricks_u16`` into each level's current device chunk row, at the block's z offset,
    :func:`fused_schedule`), the chunks of block ``b + 1`` are read by the I/O threads into pinned staging and uploaded,
    and the chunk rows that block ``b - 1`` completed are downloaded and written.

    Ordering: upload(b) -> compute(b) -> download(b); upload(b + 2) after compute(b) (it refills the same device
    buffer: ``stream_wait(upload, compute)`` right after compute(b) has been given its upload); a compute that refills
    a device row waits for the downloads enqueued so far (``stream_wait(compute, download)`` in front of the kernel: a
    level's rows alternate between two buffers and a level flushes at most once per block, so the row that used the
    buffer left two flushes ago, and with ``device_codec`` its frame fetch was enqueued a block ago).  The host touches
    a pinned buffer only behind its event slot: slot ``k`` = upload of input buffer ``k``, slot ``2 + k`` = downloads of
    the block in slot ``k``; a pinned row goes to the writers after that event and is downloaded into again only after
    ``writes[b - 2]`` has returned.

    ``decode_mode`` (``device_decode``): the I/O threads read the files and pack the Blosc frames with one task per Blosc
    block (``dsx_io_read_frames``), ``dsx_blosc_decode_device`` fills the device bricks, and the per-task statuses come
    back on the compute stream and are checked before anything of the block reaches the writers.  ``codec_mode``
    (``device_codec``): a finished row is encoded on the compute stream (``dsx_blosc_encode_device``), its offsets come
    back first, then exactly the packed frames, and the I/O threads write the byte ranges.
    """

    N_BUF = 2

    def __init__(self, eng, src, levels, arrays, block_z, io_threads, codec_mode=None, decode_mode=None, scale=(2, 2, 2),
                 digests=False):  # fmt: skip
        self.eng, self.src, self.levels, self.arrays, self.block_z = eng, src, levels, arrays, int(block_z)
        self.digests = bool(digests)
        self.scale = tuple(scale)
        self.codec_mode, self.decode_mode, self.io_threads = codec_mode, decode_mode, int(io_threads)
        self.zyx = tuple(int(n) for n in src.shape[-3:])
        self.ci = tuple(int(c) for c in src.chunks[-3:])
        _, H, W = self.zyx
        self.gi = (self.block_z // self.ci[0], -(-H // self.ci[1]), -(-W // self.ci[2]))
        self.in_brick = int(np.prod(self.ci))
        n_in = int(np.prod(self.gi))
        in_bytes = n_in * self.in_brick * 2
        self.bufs = []
        R = range(self.N_BUF)
        self.d_src = [self._dev(in_bytes) for _ in R]
        if decode_mode is not None:  # packed frames + task table replace the decompressed staging
            cap = n_in * (self.in_brick * 2 + 16)
            n_tasks = n_in * _engine.frame_tasks_per_chunk(self.in_brick * 2)
            task_bytes = n_tasks * _engine.TASK_DTYPE.itemsize
            self.packed = [self._host(cap).array((cap,), np.uint8) for _ in R]
            self.tasks = [self._host(task_bytes).array((n_tasks,), _engine.TASK_DTYPE) for _ in R]
            self.status = [self._host(4 * n_tasks).array((n_tasks,), np.int32) for _ in R]
            self.d_packed = [self._dev(cap) for _ in R]
            self.d_tasks = [self._dev(task_bytes) for _ in R]
            self.d_status = [self._dev(4 * n_tasks) for _ in R]
            self.routes = np.zeros(n_in, np.uint8)  # (one read at a time)
            self.read_info = [None] * self.N_BUF  # (packed bytes, tasks, chunk paths) of the block read into buffer k
            self.decode_info = [None] * self.N_BUF  # the same of the block SUBMITTED from buffer k (plus chunk / kind)
        else:
            self.stage_in = [self._host(in_bytes).array(self.gi + (self.in_brick,), np.uint16) for _ in R]
        # per level: two device chunk rows in brick order + what carries a finished row to the host
        self.grid, self.d_row, self.stage_row = [], [], []
        self.d_frames, self.d_offsets, self.frames, self.offsets = [], [], [], []
        for lv in levels:
            ny, nx = -(-lv.shape[1] // lv.chunks[1]), -(-lv.shape[2] // lv.chunks[2])
            brick = int(np.prod(lv.chunks))
            self.grid.append((ny, nx, brick))
            self.d_row.append([self._dev(ny * nx * brick * 2) for _ in R])
            if codec_mode is not None:
                cap = ny * nx * (brick * 2 + 16)
                self.d_frames.append([self._dev(cap) for _ in R])
                self.d_offsets.append([self._dev(8 * (ny * nx + 1)) for _ in R])
                self.frames.append([self._host(cap).array((cap,), np.uint8) for _ in R])
                self.offsets.append([self._host(8 * (ny * nx + 1)).array((ny * nx + 1,), np.int64) for _ in R])
            else:
                self.stage_row.append([self._host(ny * nx * brick * 2).array((ny, nx, brick), np.uint16) for _ in R])
        # digests: one record per chunk of a row, taken on the device and carried to the row's writer with its offsets
        self.d_dig, self.dig = [], []
        if self.digests:
            rec = _engine.DIGEST_DTYPE
            for ny, nx, _ in self.grid:
                self.d_dig.append([self._dev(ny * nx * rec.itemsize) for _ in R])
                self.dig.append([self._host(ny * nx * rec.itemsize).array((ny * nx,), rec) for _ in R])
        work = _engine.pyramid_work_bytes((self.block_z, H, W), len(levels) + 1, self.scale)
        self.d_work = self._dev(work) if work else None
        self.cur, self.flushes = [0] * len(levels), [[] for _ in R]
        self.timing = {"read_s": 0.0, "write_s": 0.0, "upload_bytes": 0, "download_bytes": 0,
                       "decode_routes": {"device": 0, "host": 0, "fill": 0}}  # fmt: skip

    def _dev(self, nbytes):
        self.bufs.append(self.eng.alloc(max(int(nbytes), 16)))
        return self.bufs[-1]

    def _host(self, nbytes):
        self.bufs.append(self.eng.alloc_host(max(int(nbytes), 16)))
        return self.bufs[-1]

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    # -- host stages (I/O threads) -------------------------------------------------------------
    def _read(self, z0, z1, k):
        """The level-0 chunks of planes ``[z0, z1)`` into pinned buffer ``k`` (decoded, or as packed frames + tasks)."""
        t0 = time.perf_counter()
        lead = (0,) * (self.src.ndim - 3)
        bz0, nbz = z0 // self.ci[0], -(-(z1 - z0) // self.ci[0])
        idx = list(itertools.product(range(nbz), range(self.gi[1]), range(self.gi[2])))
        paths = [self.src._chunk_path(lead + (bz0 + i[0], i[1], i[2])) for i in idx]
        routes = self.timing["decode_routes"]
        try:
            if self.decode_mode is not None:
                from . import zarr_destriper as zd

                pb, nt = self.eng.io_read_frames(paths, self.in_brick * 2, self.packed[k], self.tasks[k],
                                                 threads=self.io_threads, fill_value=int(self.src.fill_value),
                                                 routes=self.routes, mode=zd.ZDEC_MODES[self.decode_mode],
                                                 zlib_chunks=self.src.compressor[0] == "zlib")  # fmt: skip
                self.read_info[k] = (pb, nt, paths)
                seen = np.bincount(self.routes[: len(paths)], minlength=3)
                for name, r in (("device", _engine.ROUTE_DEVICE), ("host", _engine.ROUTE_HOST), ("fill", _engine.ROUTE_FILL)):
                    routes[name] += int(seen[r])
            else:
                stage = self.stage_in[k]
                self.eng.io_read_chunks(paths, [stage[i] for i in idx], threads=self.io_threads, codec=self.src.codec,
                                        fill_value=int(self.src.fill_value))  # fmt: skip
                there = sum(os.path.exists(p) for p in paths)
                routes["host"] += there
                routes["fill"] += len(paths) - there
        except _engine.DsxError as e:
            if e.message.startswith(("blosc:", "zlib:")):  # a malformed chunk the reader itself refused: "blosc: ... (<chunk file>)"
                raise ValueError(e.message) from None
            raise
        finally:
            self.timing["read_s"] += time.perf_counter() - t0
        return nbz

    def _write(self, flushes):
        """The chunk rows that left with a block: ``(level index, buffer, chunk row)`` each."""
        t0 = time.perf_counter()
        try:
            for i, j, row in flushes:
                arr, (ny, nx, _) = self.arrays[i], self.grid[i]
                lead = (0,) * (arr.ndim - 3)
                idx = list(itertools.product(range(ny), range(nx)))
                paths = [arr._chunk_path(lead + (row, y, x)) for y, x in idx]
                if self.codec_mode is not None:  # finished frames: chunk c is bytes [offsets[c], offsets[c + 1])
                    frames, offs = self.frames[i][j], self.offsets[i][j]
                    self.eng.io_write_chunks(paths, [frames[offs[c] : offs[c + 1]] for c in range(len(idx))],
                                             threads=self.io_threads, zlib_level=-1)  # fmt: skip
                    continue
                comp = arr.compressor
                self.eng.io_write_chunks(paths, [self.stage_row[i][j][y, x] for y, x in idx], threads=self.io_threads,
                                         zlib_level=-1 if comp is None else int(comp[1]),
                                         blosc=arr.blosc_write_params() if comp and comp[0] == "blosc" else None)  # fmt: skip
            if self.digests:  # behind the chunk files they describe
                self._write_digests(flushes)
        finally:
            self.timing["write_s"] += time.perf_counter() - t0

    def _write_digests(self, flushes):
        """(digests) The records of the rows that left with a block, each into its own range of its level's manifest."""
        for i, j, row in flushes:
            self.arrays[i].set_digest_records(row, self.dig[i][j])

    # -- device stages (asynchronous) ----------------------------------------------------------
    def _submit_in(self, k, nbz):
        """Upload(b), and with ``device_decode`` the decode: nothing here touches a device row."""
        from .engine import STREAM_COMPUTE as C, STREAM_UPLOAD as U

        eng = self.eng
        if self.decode_mode is not None:
            pb, nt, paths = self.read_info[k]
            self.decode_info[k] = (nt, self.tasks[k]["chunk"][:nt].copy(), paths, self.tasks[k]["kind"][:nt].copy())
            if pb:
                eng.copy_h2d_async(self.d_packed[k], self.packed[k][:pb], U)
            if nt:
                eng.copy_h2d_async(self.d_tasks[k], self.tasks[k][:nt], U)
            self.timing["upload_bytes"] += pb + nt * _engine.TASK_DTYPE.itemsize
        else:
            eng.copy_h2d_async(self.d_src[k], self.stage_in[k][:nbz], U)
            self.timing["upload_bytes"] += self.stage_in[k][:nbz].nbytes
        eng.event_record(k, U)  # pinned input buffer k may be refilled once this has passed
        eng.stream_wait(C, U)   # compute(b) after upload(b)
        eng.stream_wait(U, C)   # uploads from now on after compute(b - 1): they refill its buffer
        if self.decode_mode is not None:  # the bricks from the frames; the statuses come back in stream order
            eng.blosc_decode_device(self.d_packed[k], pb, self.d_tasks[k], nt, self.d_src[k], self.d_status[k])
            if nt:
                eng.copy_d2h_async(self.status[k][:nt], self.d_status[k], C)

    def _submit_out(self, z0, z1, k, shares):
        """Compute(b) and download(b): once the pinned rows of block b - 2 have been written out."""
        from .engine import STREAM_COMPUTE as C, STREAM_DOWNLOAD as D

        eng, (_, H, W), cur = self.eng, self.zyx, self.cur
        eng.stream_wait(C, D)  # (lands before the kernel:) after the downloads enqueued so far
        eng.pyramid_bricks(self.d_src[k], (z1 - z0, H, W), self.ci, [lv.chunks for lv in self.levels],
                           [self.d_row[i][cur[i]] for i in range(len(shares))], z0s=[s.offset for s in shares],
                           zero=[s.first for s in shares], rows=[1] * len(shares), d_work=self.d_work,
                           **({} if self.scale == (2, 2, 2) else {"scale": self.scale}))  # (the default: the call as it always was)
        flushes = []
        for i, s in enumerate(shares):
            if not s.flush:
                continue
            j = cur[i]
            if self.digests:  # the finished row where it lies, before the encoder reads it
                lv = self.levels[i]
                eng.brick_digest(self.d_row[i][j], (1,) + self.grid[i][:2], lv.chunks,
                                 (min(lv.chunks[0], lv.shape[0] - s.row * lv.chunks[0]),) + tuple(lv.shape[1:]), self.d_dig[i][j])
            if self.codec_mode is not None:
                ny, nx, brick = self.grid[i]
                eng.blosc_encode_device(self.d_row[i][j], ny * nx, brick * 2, self.d_frames[i][j], self.d_offsets[i][j],
                                        typesize=2, clevel=int(self.arrays[i].compressor[1]), mode=self.codec_mode)  # fmt: skip
            flushes.append((i, j, s.row))
            cur[i] = (j + 1) % self.N_BUF
        self.flushes[k] = flushes
        eng.stream_wait(D, C)  # download(b) after compute(b)
        for i, j, _ in flushes:
            if self.codec_mode is not None:
                eng.copy_d2h_async(self.offsets[i][j], self.d_offsets[i][j], D)
            else:
                eng.copy_d2h_async(self.stage_row[i][j], self.d_row[i][j], D)
                self.timing["download_bytes"] += self.stage_row[i][j].nbytes
            if self.digests:
                eng.copy_d2h_async(self.dig[i][j], self.d_dig[i][j], D)
                self.timing["download_bytes"] += self.dig[i][j].nbytes
        eng.event_record(self.N_BUF + k, D)  # the rows (or their frame offsets) and the statuses of block b are here

    def _fetch_frames(self, k):
        """(device codec; the offsets of the rows of the block in slot k are on the host) Download exactly their frames."""
        from .engine import STREAM_DOWNLOAD as D

        for i, j, _ in self.flushes[k]:
            offs = self.offsets[i][j]
            total = int(offs[-1])
            self.timing["download_bytes"] += total + offs.nbytes
            if total:
                self.eng.copy_d2h_async(self.frames[i][j][:total], self.d_frames[i][j], D)
        self.eng.event_record(self.N_BUF + k, D)
        self.eng.event_sync(self.N_BUF + k)

    def _check_decode(self, k):
        """(device decode; the block in slot k has been computed) A malformed frame raises as the level-0 pass does."""
        if self.decode_mode is None:
            return
        nt, chunk, paths, kinds = self.decode_info[k]
        st = self.status[k][:nt]
        bad = np.flatnonzero(st)
        if bad.size:
            from . import zarr_destriper as zd

            i = int(bad[0])
            raise ValueError(zd.bad_stream_message(int(kinds[i]), paths[int(chunk[i])], int(st[i]),
                                                   self.src.compressor[0] == "zlib"))  # fmt: skip

    def _finish(self, k, writer, writes):
        """Block in slot k: wait for its downloads, check its statuses, then hand its rows to the writers."""
        self.eng.event_sync(self.N_BUF + k)
        self._check_decode(k)
        if self.codec_mode is not None:
            self._fetch_frames(k)
        writes.append(writer.submit(self._write, list(self.flushes[k])))

    def run(self):
        """All blocks of level 0 through the pipeline; returns the number of blocks."""
        sched = fused_schedule(self.levels, 0, self.zyx[0], self.block_z, self.scale)
        nb, N = len(sched), self.N_BUF
        self.cur = [0] * len(self.levels)
        reader = ThreadPoolExecutor(max_workers=1)  # stage drivers: one read and one write in flight,
        writer = ThreadPoolExecutor(max_workers=1)  # each fanning its chunks out over the I/O pool
        try:
            reads = {b: reader.submit(self._read, *sched[b][0], b % N) for b in range(min(N, nb))}
            writes = []
            for b in range(nb):
                k = b % N
                (z0, z1), shares = sched[b]
                nbz = reads.pop(b).result()
                self._submit_in(k, nbz)
                if b >= N:
                    writes[b - N].result()  # the pinned rows of slot k have been written out
                self._submit_out(z0, z1, k, shares)
                if b + N < nb:
                    self.eng.event_sync(k)  # upload(b) has left pinned input buffer k
                    reads[b + N] = reader.submit(self._read, *sched[b + N][0], k)
                if b >= 1:
                    self._finish((b - 1) % N, writer, writes)
            if nb:
                self._finish((nb - 1) % N, writer, writes)
            for w in writes:
                w.result()
        finally:
            reader.shutdown()
            writer.shutdown()
        return nb


def _write_pipelined(level0_path, group_path, n_levels, chunks, compressor, device, device_codec, device_decode, io_threads,
                     scale=(2, 2, 2), digests=False):  # fmt: skip
    from . import zarr_destriper as zd

    t_start = time.perf_counter()
    codec_mode = zd.output_codec_mode(device_codec, compressor)  # "lz4" for Blosc-LZ4 levels
    decode_mode = zd.device_decode_mode(device_decode)
    src = MiniZarrArray.open(level0_path)
    if src.dtype != np.uint16 or any(n != 1 for n in src.shape[:-3]):
        raise ValueError("the pyramid kernel takes uint16 volumes with singleton leading axes")
    if decode_mode is not None and not zd.device_decode_input_ok(src, decode_mode):
        raise ValueError("device_decode needs a Blosc uint16 input, not {!r} {}".format(src.compressor, src.dtype))
    zyx, lead = tuple(src.shape[-3:]), tuple(src.shape[:-3])
    levels = fused_levels(zyx, chunks, n_levels, scale)
    block_z = pipelined_block_z(src.chunks[-3], levels, scale) if levels else None
    arrays, shapes = [], []
    for lv in levels:  # created as the slab route creates them
        out_shape = lead + lv.shape
        ck = tuple(min(c, n) for c, n in zip(tuple(chunks)[-len(out_shape):], out_shape))
        if len(ck) != len(out_shape) or ck[-3:] != lv.chunks:
            raise ValueError("chunks {} do not cover the axes of a level of shape {}".format(tuple(chunks), out_shape))
        arrays.append(MiniZarrArray.create(os.path.join(group_path, str(lv.level)), out_shape, ck, np.uint16,
                                           compressor=compressor, dimension_separator="/", digests=digests))  # fmt: skip
        shapes.append(out_shape)
    if codec_mode is not None and arrays:
        if not zd.device_codec_output_ok(arrays[0]):
            raise ValueError("device_codec needs a Blosc-zstd or Blosc-LZ4 uint16 output with byte shuffle, not {!r}"
                             .format(arrays[0].compressor))
    if io_threads is None:
        io_threads = zd.default_io_threads(1)
    LAST_PYRAMID.clear()
    LAST_PYRAMID.update(route="pipelined", block_z=block_z, levels=[lv.level for lv in levels], decode_routes=None, scale=scale,
                        read_s=0.0, write_s=0.0, upload_bytes=0, download_bytes=0, seconds=None, digests=bool(digests))  # fmt: skip
    if levels:
        eng = _engine.DestripeEngine(device)
        pipe = None
        try:
            pipe = _PipelinedPyramid(eng, src, levels, arrays, block_z, io_threads, codec_mode, decode_mode, scale, digests)
            try:
                pipe.run()
            finally:
                LAST_PYRAMID.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in pipe.timing.items()})
            eng.sync()
        finally:
            if pipe is not None:
                try:
                    eng.sync()  # nothing in flight reads or writes a buffer that is about to be freed
                except Exception:  # noqa: BLE001 - the error that brought us here is the one to report
                    pass
                pipe.close()
            eng.close()
    LAST_PYRAMID["seconds"] = time.perf_counter() - t_start
    return shapes
