"""Multiscale pyramid of the destriped volume on the GPU.

Mirrors ``compute_pyramid`` (``/root/reference/code/aind_smartspim_destripe/zarr_destriper.py:365-407``) and the
level loop of ``compute_multiscale`` (``:677-794``): ``xarray_multiscale.multiscale`` with the
``windowed_mean`` reducer, ``scale_factors`` 2 per spatial axis and ``preserve_dtype=True`` -- every level
is the 2 x 2 x 2 windowed mean of the previous one, truncated back to uint16 -- without the dask
``LocalCluster`` (``:689-697``): one HIP kernel per level (``dsx_downsample2_u16``), the volume stays in HBM
between levels.  No CPU fallback.
"""

from collections import namedtuple

import numpy as np

from . import engine as _engine
from .distributed import z_shard
from .mini_zarr import MiniZarrArray


def _check_scale(scale_axis):
    scale = [int(s) for s in scale_axis]
    if len(scale) < 3 or any(s != 1 for s in scale[:-3]) or scale[-3:] != [2, 2, 2]:
        raise ValueError("only scale factors (.., 2, 2, 2) are implemented (production setting, zarr_destriper.py:1176)")


# ---- the pyramid fused into the destripe pass (zarr_destriper.destripe_zarr_store(pyramid_group=...)) -----------------
# One level of the plan: its index, its [Z, Y, X] shape and its chunk shape (clamped to the shape).
FusedLevel = namedtuple("FusedLevel", "level shape chunks")
# One level's share of one z block: chunk row, first plane inside the row, planes, whether the block is the first to
# touch the row (the row must be zeroed) and whether the row leaves after this block.
BlockShare = namedtuple("BlockShare", "level row offset planes first flush")


def fused_levels(zyx, chunks, n_levels):
    """Levels ``1 .. n_levels - 1`` as :func:`write_pyramid_levels` writes them: shape ``n // 2`` of the previous
    level, chunks ``min(c, n)``, stopping at a source level with an axis shorter than 2."""
    levels, cur = [], tuple(int(n) for n in zyx)
    for i in range(1, int(n_levels)):
        if min(cur) < 2:
            break
        cur = tuple(n // 2 for n in cur)
        levels.append(FusedLevel(i, cur, tuple(min(int(c), n) for c, n in zip(tuple(chunks)[-3:], cur))))
    return levels


def fused_z_chunk(z_chunk, levels):
    """z alignment of the rank shards: one chunk row of the deepest level, in level-0 planes
    (``cz << (levels written - 1)``), so that every chunk of every level is written by exactly one rank."""
    return int(z_chunk) << len(levels)


def fused_z_range(n_slices, world_size, rank, z_chunk, levels):
    return z_shard(n_slices, world_size, rank, z_chunk=fused_z_chunk(z_chunk, levels))


def fused_check_blocks(levels, block_z):
    """``ValueError`` unless z blocks of ``block_z`` planes hold whole windows of every level and fill whole chunk rows."""
    if levels and block_z % (1 << len(levels)):
        raise ValueError("fused_pyramid needs z blocks of a multiple of {} planes (2 x 2 x 2 windows of {} levels), "
                         "not {}".format(1 << len(levels), len(levels), block_z))  # fmt: skip
    for lv in levels:
        if lv.shape[0] > lv.chunks[0] and (lv.chunks[0] << lv.level) % block_z:
            raise ValueError("fused_pyramid needs z blocks that fill whole chunk rows of every level: {} planes do not "
                             "divide the {} of a level-{} chunk row".format(block_z, lv.chunks[0] << lv.level, lv.level))  # fmt: skip


def fused_schedule(levels, z_start, z_stop, block_z):
    """What every z block of ``[z_start, z_stop)`` (a :func:`fused_z_range`) gives to every level:
    ``[((z0, z1), [BlockShare per level])]``.  A chunk row leaves (``flush``) with the block that completes it, or with
    the last block of the range when it holds anything."""
    out, filled = [], [0] * len(levels)
    starts = list(range(z_start, z_stop, block_z))
    for z0 in starts:
        z1, shares = min(z0 + block_z, z_stop), []
        for i, lv in enumerate(levels):
            p0, n, cz = z0 >> lv.level, (min(z0 + block_z, z_stop) - z0) >> lv.level, lv.chunks[0]
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


def compute_pyramid(data, n_lvls, scale_axis, chunks="auto", device=0, engine=None):
    """``zarr_destriper.py:365-407``: ``[level 0 (the input), level 1, ...]``, ``n_lvls`` entries.

    ``data``: uint16 with the spatial axes last (``[Z, Y, X]`` up to ``[1, 1, Z, Y, X]``; leading axes must be
    singletons); ``chunks`` is accepted for signature parity and ignored (dense arrays come back).
    """
    _check_scale(scale_axis)
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
            if min(zyx) < 2:
                break
            nxt = tuple(n // 2 for n in zyx)
            d_next = eng.alloc(max(int(np.prod(nxt)) * 2, 16))
            bufs.append(d_next)
            eng.downsample2(d_prev, d_next, zyx)
            levels.append(d_next.download(nxt, np.uint16).reshape(lead + nxt))
            d_prev, zyx = d_next, nxt
    finally:
        for b in bufs:
            b.free()
        if engine is None:
            eng.close()
    return levels


def write_pyramid_levels(level0_path, group_path, scale_factor=(2, 2, 2), n_levels=3, chunks=(1, 1, 64, 128, 128),
                       compressor="blosc", device=0, slab_planes=None):  # fmt: skip
    """Level loop of ``compute_multiscale`` (``zarr_destriper.py:746-782``) over Zarr-v2 directory stores
    (``zarr_destriper.compute_multiscale`` is the entry point with the reference's signature and calls this):
    writes ``<group_path>/<i>`` for ``i = 1 .. n_levels - 1`` (uint16, ``"/"`` separator), every level from the
    previous one.  OME-NGFF metadata (``:728-742``) is out of scope.  Returns the written arrays' shapes.

    The volume is streamed in z-slabs (a 34 GB channel does not fit one allocation, nor host RAM twice):
    a slab of ``2 * output z-chunk`` source planes is read, reduced by one ``dsx_downsample2_u16`` launch
    and written as whole output chunks; the 2 x 2 x 2 windows never straddle a slab because slabs start
    at even planes.
    """
    import os

    _check_scale((1,) * 2 + tuple(scale_factor))
    eng = _engine.DestripeEngine(device)
    shapes = []
    try:
        src_path = level0_path
        for i in range(1, int(n_levels)):
            src = MiniZarrArray.open(src_path)
            if src.dtype != np.uint16 or any(n != 1 for n in src.shape[:-3]):
                raise ValueError("the pyramid kernel takes uint16 volumes with singleton leading axes")
            Z, Y, X = src.shape[-3:]
            if min(Z, Y, X) < 2:
                break
            out_zyx = (Z // 2, Y // 2, X // 2)
            lead = src.shape[:-3]
            out_shape = lead + out_zyx
            ck = tuple(min(c, n) for c, n in zip(tuple(chunks)[-len(out_shape):], out_shape))
            dst = MiniZarrArray.create(os.path.join(group_path, str(i)), out_shape, ck, np.uint16,
                                       compressor=compressor, dimension_separator="/")  # fmt: skip
            slab = int(slab_planes) if slab_planes else 2 * ck[-3]
            slab += slab & 1
            d_src = eng.alloc(slab * Y * X * 2)
            d_dst = eng.alloc(max((slab // 2) * out_zyx[1] * out_zyx[2] * 2, 16))
            try:
                lead_idx = (0,) * len(lead)
                for z in range(0, 2 * out_zyx[0], slab):
                    n = min(slab, 2 * out_zyx[0] - z)  # even: an odd trailing plane is cropped
                    d_src.upload(src[lead_idx + (slice(z, z + n),)])
                    eng.downsample2(d_src, d_dst, (n, Y, X))
                    out = d_dst.download((n // 2,) + out_zyx[1:], np.uint16)
                    dst[lead_idx + (slice(z // 2, z // 2 + n // 2),)] = out
            finally:
                d_src.free()
                d_dst.free()
            shapes.append(out_shape)
            src_path = os.path.join(group_path, str(i))
    finally:
        eng.close()
    return shapes
