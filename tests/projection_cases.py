"""Inputs of the projection tests (``tests/test_projections_host.py``, ``tests/test_gpu_projections.py``): built once,
never modified.  Every case is ``(name, buffer, first plane, planes)`` -- the planes of the uint16 ``[Z, H, W]`` buffer
that are projected; what lies outside them holds values that do not occur inside.  Expected values are
``projections.project_volume`` of those planes, that is NumPy: the sums make every dropped or doubled voxel visible, the
maxima every stray one."""

import functools

import numpy as np

from aind_smartspim_destripe_amd import projections as pr

SENTINEL = 65535  # guard value around the sub-ranges of case (d)
ODD = (3, 37, 53)  # neither a multiple of the 8-voxel vector nor of a tile; a 2-byte row pitch


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def odd_permutation():
    """(a) 3 x 37 x 53: a permutation of distinct values scaled over the full range (the scalar body)."""
    n = int(np.prod(ODD))
    v = (np.arange(n, dtype=np.uint64) * 65535 // (n - 1)).astype(np.uint16)
    assert np.unique(v).size == n and v[-1] == 65535
    return _frozen(np.random.RandomState(21).permutation(v).reshape(ODD))


@functools.lru_cache(maxsize=None)
def wide_random():
    """(b) 5 x 40 x 1032 random full range: the vector body, two column strips of 512 plus one 8-pixel remainder, two
    row tiles of 32 (the second with 8 rows)."""
    return _frozen(np.random.RandomState(22).randint(0, 65536, (5, 40, 1032)))


@functools.lru_cache(maxsize=None)
def constant(value):
    """(c) 4 x 64 x 128 of one value: with 65 535 the sums reach W, H and Z times 65 535."""
    return _frozen(np.full((4, 64, 128), value))


@functools.lru_cache(maxsize=None)
def guarded():
    """(d) four planes of 37 x 53: planes 0 and 3 hold only SENTINEL, planes 1 and 2 values below 60 000.  Planes [1:3)
    and [1:2) start 37 * 53 * 2 = 3922 bytes into the buffer: 2-byte aligned, 2 bytes past a 16-byte boundary.  Any read
    outside the range shows up in a maximum."""
    rs = np.random.RandomState(23)
    buf = np.full((4,) + ODD[1:], SENTINEL, np.uint16)
    buf[1] = rs.randint(0, 60000, ODD[1:])
    buf[2] = rs.randint(0, 60000, ODD[1:])
    return _frozen(buf)


@functools.lru_cache(maxsize=None)
def random_volume(shape, seed):
    """(e) degenerate shapes, (f) production row pitches."""
    return _frozen(np.random.RandomState(seed).randint(0, 65536, shape))


def cases():
    g = guarded()
    out = [
        ("a_odd_permutation", odd_permutation(), 0, ODD[0]),
        ("b_wide_random", wide_random(), 0, 5),
        ("c_constant_65535", constant(65535), 0, 4),
        ("c_constant_0", constant(0), 0, 4),
        ("d_planes_1_3", g, 1, 2),
        ("d_planes_1_2", g, 1, 1),
    ]
    for i, shape in enumerate([(1, 1, 1), (1, 1, 600), (1, 600, 1), (9, 1, 8)]):
        out.append(("e_{}x{}x{}".format(*shape), random_volume(shape, 30 + i), 0, shape[0]))
    for i, shape in enumerate([(2, 16, 2000), (2, 16, 1800)]):
        out.append(("f_{}x{}x{}".format(*shape), random_volume(shape, 40 + i), 0, shape[0]))
    return out


def seven_planes():
    """7 x 37 x 53 random full range, for the accumulation over blocks of 4 and 3 planes."""
    return random_volume((7,) + ODD[1:], 50)


def wide_seven():
    """7 x 40 x 1032: the same through the vector body."""
    return random_volume((7, 40, 1032), 51)


@functools.lru_cache(maxsize=None)
def _expected(name):
    for n, buf, z0, nz in cases():
        if n == name:
            got = pr.project_volume(buf[z0 : z0 + nz])
            for a in got.values():
                a.setflags(write=False)
            return got
    raise KeyError(name)


def expected(name):
    """``project_volume`` of the case's planes, computed once and shared."""
    return _expected(name)


CANARY = {"max_y": 0xABCD, "sum_y": 0xDEADBEEF, "max_x": 0xABCD, "sum_x": 0xDEADBEEF}


def canary_arrays(zyx):
    """The six arrays of a ``zyx`` volume: zeros for the z arrays, a canary in every row of the others."""
    from aind_smartspim_destripe_amd import engine

    return {name: np.full(shape, CANARY.get(name, 0), dtype) for name, shape, dtype in engine.projection_shapes(zyx)}
