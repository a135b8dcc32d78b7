"""Inputs of the voxel-histogram tests (``tests/test_volhist_host.py``, ``tests/test_gpu_volhist.py``): built once,
never modified.  Every case is ``(name, buffer, start voxel, voxel count)`` -- the range of the flat uint16 buffer that
is counted; what lies outside it holds values that do not occur inside."""

import functools

import numpy as np

BINS = 65536
SENTINEL = 65535  # guard value around the sub-ranges of case (e)
ODD = (3, 37, 53)  # neither a multiple of the 8-voxel vector nor of the block size


@functools.lru_cache(maxsize=None)
def window_edges():
    """(a) every value 0 .. 65535 present ``1 + (v % 3)`` times, shuffled: both ends of the range and every edge of
    whatever LDS window the kernel uses."""
    v = np.arange(BINS, dtype=np.uint16)
    buf = np.repeat(v, 1 + (np.arange(BINS) % 3))
    np.random.RandomState(11).shuffle(buf)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def odd_random():
    """(b) 3 x 37 x 53 random full-range voxels."""
    buf = np.random.RandomState(12).randint(0, BINS, ODD).astype(np.uint16)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def constant(value):
    """(c) 8 x 512 x 512 voxels of one value: every lane of every wave hits one bin."""
    buf = np.full((8, 512, 512), value, np.uint16)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def guarded():
    """(e) planes of the odd size of (b) with guards: plane 0 and plane 3 hold only SENTINEL, plane 1 values below
    30 000, plane 2 values in [30 000, 60 000).  Planes [1:3] and [1:2] start 37 * 53 * 2 = 3922 bytes into the buffer:
    2-byte aligned, 2 bytes past a 16-byte boundary."""
    rs = np.random.RandomState(13)
    buf = np.full((4,) + ODD[1:], SENTINEL, np.uint16)
    buf[1] = rs.randint(0, 30000, ODD[1:])
    buf[2] = rs.randint(30000, 60000, ODD[1:])
    buf.setflags(write=False)
    return buf


def cases():
    plane = ODD[1] * ODD[2]
    a, b, g = window_edges(), odd_random(), guarded()
    return [
        ("a_window_edges", a, 0, a.size),
        ("b_odd_sizes", b, 0, b.size),
        ("c_constant_150", constant(150), 0, constant(150).size),
        ("c_constant_40000", constant(40000), 0, constant(40000).size),
        ("e_planes_1_3", g, plane, 2 * plane),
        ("e_planes_1_2", g, plane, plane),
    ]


def expected(buf, start, count):
    return np.bincount(buf.reshape(-1)[start : start + count], minlength=BINS).astype(np.int64)
