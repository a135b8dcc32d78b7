"""Cases shared by the tests of the pyramid with a scale factor of 1 or 2 per axis (``test_pyramid_scale_host.py``,
``test_gpu_pyramid_scale.py``): the factor sets, block volumes with sums near the maximum, and the oracle's levels of a
block in brick order."""

import itertools

import numpy as np

from aind_smartspim_destripe_amd import pyramid
from oracle import format_oracle as fo

# every (fz, fy, fx) of 1 or 2 but (1, 1, 1); (2, 2, 2) is the production setting and runs the kernels it always ran
SCALES = [s for s in itertools.product((1, 2), repeat=3) if s != (1, 1, 1)]
BLOCKS = [(8, 20, 44), (6, 10, 12), (7, 9, 11), (64, 36, 50)]
BASES = [(64, 128, 128), (4, 8, 8), (3, 5, 7)]


def scale_id(scale):
    return "x".join(str(f) for f in scale)


def block_volume(zyx, seed=0):
    rs = np.random.RandomState(sum(zyx) + seed)
    vol = rs.randint(0, 65536, zyx).astype(np.uint16)
    vol[: zyx[0] // 2 + 1, : zyx[1] // 2 + 1] |= 0xFFF0  # window sums near 8 * 65535
    return vol


def extents(zyx, level, scale):
    """Shape of level ``level`` of a block ``zyx``: ``previous // f`` per axis, ``level`` times."""
    return tuple(int(n) // int(f) ** level for n, f in zip(zyx, scale))


def level_chunks(zyx, base, n_levels, scale, vol_z=None):
    """Chunk shapes of the levels with a non-empty share of the block ``zyx`` inside a volume of ``vol_z`` planes (the
    block itself by default): ``base`` clamped to the volume's level, as ``fused_levels`` plans them."""
    levels = pyramid.fused_levels((vol_z or zyx[0],) + tuple(zyx[1:]), base, n_levels, scale)
    return [lv.chunks for lv in levels if min(extents(zyx, lv.level, scale)) > 0]


def expected_bricks(vol, chunks, z0s, rows, scale):
    """Per level: the oracle's level of the block in brick order at its z offset, ``rows`` chunk rows."""
    pyr = fo.pyramid(vol, len(chunks) + 1, scale)
    out = []
    for lvl, (ck, z0, r) in enumerate(zip(chunks, z0s, rows), start=1):
        b = fo.planes_to_bricks(pyr[lvl], ck, z0)
        full = np.zeros((r,) + b.shape[1:], np.uint16)
        full[: b.shape[0]] = b
        out.append(full)
    return out


def source_bricks(vol, src_chunk, poison=True):
    """The block in the chunk order of an array with chunks ``src_chunk``; ``poison``: 0xFFFF wherever a brick sticks out
    of the block."""
    bricks = fo.planes_to_bricks(vol, src_chunk)
    if poison:
        bricks[fo.planes_to_bricks(np.ones(vol.shape, np.uint8), src_chunk) == 0] = 0xFFFF
    return bricks
