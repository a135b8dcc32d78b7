"""Cases of the chunk digest (``csrc/dsx_digest.h``) shared by the host and the GPU tests, and its restatement in NumPy
uint64 arithmetic (which wraps mod 2^64 as the contract asks).

Chunk shapes at the smallest sizes where the kernel's bodies and seams differ: one voxel; a row shorter than a vector;
whole vectors (the 16-byte body); 130 = 16 vectors + 2 voxels (the 2-byte body, two column lanes idle); 1024 = 128
column lanes, two rows in flight; 4104 = two column passes of 256 lanes, the second ragged, 8-voxel aligned; and
(40, 16, 8): 640 rows, two row segments of one brick (the partials of two blocks meet in one record).
"""

import itertools

import numpy as np

MASK = (1 << 64) - 1
COL_BASE = 1 << 32

CHUNKS = [(1, 1, 1), (2, 3, 5), (4, 8, 16), (3, 5, 130), (2, 2, 1024), (1, 3, 4104), (40, 16, 8)]
DATA = ["zeros", "ones", "random", "high"]


def m_int(k):
    """The weight in Python integers."""
    z = ((k + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return (z ^ (z >> 31)) | 1


def m_np(k):
    """The weight of every element of a uint64 array."""
    with np.errstate(over="ignore"):
        z = (np.asarray(k, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (z ^ (z >> np.uint64(31))) | np.uint64(1)


def restate(chunk, extents=None):
    """``(count, sum, wsum)`` of a uint16 ``chunk`` of shape ``(c0, c1, c2)`` with valid ``extents``, as Python ints."""
    chunk = np.asarray(chunk)
    c0, c1, c2 = chunk.shape
    e0, e1, e2 = extents if extents is not None else chunk.shape
    v = chunk[:e0, :e1, :e2].astype(np.uint64)
    rows = (np.arange(e0, dtype=np.uint64)[:, None] * np.uint64(c1) + np.arange(e1, dtype=np.uint64)[None, :])
    with np.errstate(over="ignore"):
        dot = (v * m_np(np.uint64(COL_BASE) + np.arange(e2, dtype=np.uint64))[None, None, :]).sum(axis=2, dtype=np.uint64)
        wsum = (m_np(rows) * dot).sum(dtype=np.uint64)
        total = v.sum(dtype=np.uint64)
    return (e0 * e1 * e2, int(total), int(wsum))


def restate_int(chunk, extents=None):
    """The same in Python integers (small chunks)."""
    chunk = np.asarray(chunk)
    c0, c1, c2 = chunk.shape
    e0, e1, e2 = extents if extents is not None else chunk.shape
    s = w = 0
    for i0, i1 in itertools.product(range(e0), range(e1)):
        dot = sum(int(chunk[i0, i1, i2]) * m_int(COL_BASE + i2) for i2 in range(e2))
        s += sum(int(x) for x in chunk[i0, i1, :e2])
        w += m_int(i0 * c1 + i1) * dot
    return (e0 * e1 * e2, s & MASK, w & MASK)


def restate_array(volume, chunks):
    """Records of every chunk of a ``(Z, Y, X)`` uint16 ``volume`` cut into ``chunks``, as a list of int triples in C
    order of the chunk grid.  (Padding is given another value than any fill: it must not matter.)"""
    Z, Y, X = volume.shape
    out = []
    for g in itertools.product(*[range(-(-n // c)) for n, c in zip(volume.shape, chunks)]):
        e = tuple(min(c, n - i * c) for c, n, i in zip(chunks, volume.shape, g))
        brick = np.full(chunks, 0xABCD, np.uint16)
        brick[: e[0], : e[1], : e[2]] = volume[tuple(slice(i * c, i * c + k) for i, c, k in zip(g, chunks, e))]
        out.append(restate(brick, e))
    return out


def all_short(c):
    """Short by one on every axis (where the axis has more than one voxel)."""
    return tuple(max(1, x - 1) for x in c)


def extents_of(c):
    """Full; short by one on each axis separately and together; (1, 1, 1) -- deduplicated, every extent >= 1."""
    c0, c1, c2 = c
    want = [c, (c0 - 1, c1, c2), (c0, c1 - 1, c2), (c0, c1, c2 - 1), (c0 - 1, c1 - 1, c2 - 1), (1, 1, 1)]
    out = []
    for e in want:
        e = tuple(max(1, x) for x in e)
        if e not in out:
            out.append(e)
    return out


def data(kind, n, seed=0):
    rng = np.random.default_rng(1234 + seed)
    if kind == "zeros":
        return np.zeros(n, np.uint16)
    if kind == "ones":
        return np.full(n, 65535, np.uint16)
    if kind == "high":
        return rng.integers(0x8000, 0x10000, n, dtype=np.uint16)
    return rng.integers(0, 0x10000, n, dtype=np.uint16)


def brick_cases():
    """``(id, flat buffer, first element, chunk shape, extents)``: one brick at ``buffer[first:]``.  With ``first == 1``
    the brick starts one element behind an aligned base: the 2-byte body."""
    out = []
    for ci, c in enumerate(CHUNKS):
        n = int(np.prod(c))
        for ei, e in enumerate(extents_of(c)):
            for kind in DATA if e in (tuple(c), all_short(c)) else ["random"]:
                out.append(("c{}x{}x{}-e{}x{}x{}-{}".format(*c, *e, kind), data(kind, n, ci * 16 + ei), 0, c, e))
        out.append(("c{}x{}x{}-full-offset1".format(*c), data("random", n + 1, ci + 100), 1, c, c))
        e = all_short(c)
        out.append(("c{}x{}x{}-short-offset1".format(*c), data("high", n + 1, ci + 200), 1, c, e))
    return out


GRID = (2, 3, 2)


def grid_cases():
    """``(id, flat buffer, first element, chunk shape, valid)``: 2 x 3 x 2 bricks whose last brick is ragged on every
    axis (``valid`` ends one voxel, or most of a chunk, inside it)."""
    out = []
    for ci, c in enumerate(CHUNKS):
        n = int(np.prod(GRID)) * int(np.prod(c))
        short = tuple(g * x - 1 if x > 1 else g * x for g, x in zip(GRID, c))
        most = tuple((g - 1) * x + 1 for g, x in zip(GRID, c))
        for name, v in (("short1", short), ("most", most)):
            for first in (0, 1):
                out.append(("grid-c{}x{}x{}-{}-off{}".format(*c, name, first), data("random", n + first, 300 + ci), first, c, v))
    return out


def restate_grid(flat, first, c, valid, grid=GRID):
    """Records of a grid case as a list of int triples."""
    n = int(np.prod(c))
    bricks = flat[first : first + int(np.prod(grid)) * n].reshape(grid + tuple(c))
    out = []
    for g in itertools.product(*[range(x) for x in grid]):
        e = tuple(min(x, v - i * x) for x, v, i in zip(c, valid, g))
        out.append(restate(bricks[g], e))
    return out


def as_triples(records):
    """``engine.DIGEST_DTYPE`` records as a list of int triples."""
    return [(int(r["count"]), int(r["sum"]), int(r["wsum"])) for r in np.asarray(records).reshape(-1)]
