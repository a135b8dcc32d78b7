"""``k_brick_digest_u16`` (``csrc/dsx_digest.h``) on the device against its host build, exactly, on every case of
``digest_cases.py``: single bricks with full and ragged extents, bases one element off a 16-byte boundary (the 2-byte
body), grids of 2 x 3 x 2 bricks ragged on every axis; then the streams it may be enqueued on, the argument rules, and
one brick of more than 2^31 bytes."""

import ctypes

import numpy as np
import pytest

import digest_cases as dc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu

DSX_EINVAL = -1
BRICKS, GRIDS = dc.brick_cases(), dc.grid_cases()
REC = eng_mod.DIGEST_DTYPE.itemsize


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reference():
    """The host build's records of every case, computed once."""
    ref = {name: eng_mod.brick_digest_ref(buf[first:], (1, 1, 1), c, e) for name, buf, first, c, e in BRICKS}
    ref.update({name: eng_mod.brick_digest_ref(buf[first:], dc.GRID, c, v) for name, buf, first, c, v in GRIDS})
    return ref


def _device_records(e, buf, first, grid, c, v, stream=eng_mod.STREAM_COMPUTE):
    n = int(np.prod(grid))
    d, d_out = e.alloc(max(buf.nbytes, 16)), e.alloc((n + 2) * REC)
    try:
        d.upload(buf)
        d_out.upload(np.full((n + 2) * 3, 0x5A5A5A5A5A5A5A5A, np.uint64))  # the call zeroes its records, and only those
        e.brick_digest(d.ptr + 2 * first, grid, c, v, d_out, stream=stream, offset=REC)
        e.stream_sync(stream)
        got = d_out.download((n + 2,), eng_mod.DIGEST_DTYPE)
        guard = np.array([(0x5A5A5A5A5A5A5A5A,) * 3], eng_mod.DIGEST_DTYPE)[0]
        assert got[0] == guard and got[-1] == guard
        return got[1:-1]
    finally:
        d.free()
        d_out.free()


@pytest.mark.parametrize("name,buf,first,c,e", BRICKS, ids=[b[0] for b in BRICKS])
def test_device_brick_is_the_host_build(eng, reference, name, buf, first, c, e):
    got = _device_records(eng, buf, first, (1, 1, 1), c, e)
    assert dc.as_triples(got) == dc.as_triples(reference[name])


@pytest.mark.parametrize("name,buf,first,c,v", GRIDS, ids=[g[0] for g in GRIDS])
def test_device_grid_is_the_host_build(eng, reference, name, buf, first, c, v):
    got = _device_records(eng, buf, first, dc.GRID, c, v)
    assert dc.as_triples(got) == dc.as_triples(reference[name])


def test_every_stream_and_repeated_calls(eng, reference):
    name, buf, first, c, v = GRIDS[6]
    for stream in (eng_mod.STREAM_COMPUTE, eng_mod.STREAM_UPLOAD, eng_mod.STREAM_DOWNLOAD, eng_mod.STREAM_COMPUTE):
        got = _device_records(eng, buf, first, dc.GRID, c, v, stream=stream)
        assert dc.as_triples(got) == dc.as_triples(reference[name])


def test_production_brick_and_many_row_segments(eng):
    """One (64, 128, 128) brick, as the store pass writes: 16 row segments meet in one record; its z extent ragged."""
    c = (64, 128, 128)
    buf = dc.data("random", int(np.prod(c)), 77)
    for e in (c, (37, 128, 128), (64, 127, 121)):
        got = _device_records(eng, buf, 0, (1, 1, 1), c, e)
        assert dc.as_triples(got) == dc.as_triples(eng_mod.brick_digest_ref(buf, (1, 1, 1), c, e)) == [dc.restate(buf.reshape(c), e)]


def test_brick_of_two_to_the_31_voxels(eng):
    """The largest brick the call takes, 2^31 voxels = 4 GiB: offsets past 2^31 elements and 2^32 bytes.  Filled on the
    device from one uploaded row pattern, so that the host build of ONE row block gives the expected record."""
    c = (1 << 10, 1 << 10, 1 << 11)
    n = int(np.prod(c))
    tile = dc.data("random", 1 << 22, 5)  # 8 MiB, repeated 512 times
    d, d_out = eng.alloc(2 * n), eng.alloc(REC)
    try:
        for k in range(n // tile.size):
            d.upload(tile, offset=2 * k * tile.size)
        eng.brick_digest(d, (1, 1, 1), c, (c[0], c[1] - 1, c[2] - 3), d_out)
        eng.stream_sync(eng_mod.STREAM_COMPUTE)
        got = d_out.download((1,), eng_mod.DIGEST_DTYPE)
    finally:
        d.free()
        d_out.free()
    # rows r = i0 * c1 + i1; the tile holds 2048 rows, so row r has the voxels of tile row r % 2048
    e1, e2 = c[1] - 1, c[2] - 3
    rows = tile.reshape(2048, c[2])[:, :e2].astype(np.uint64)
    with np.errstate(over="ignore"):
        dot = (rows * dc.m_np(np.uint64(dc.COL_BASE) + np.arange(e2, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
        r = np.arange(c[0] * c[1], dtype=np.uint64)
        valid = (r % np.uint64(c[1])) < np.uint64(e1)
        wsum = (dc.m_np(r[valid]) * dot[(r[valid] % np.uint64(2048)).astype(np.int64)]).sum(dtype=np.uint64)
        total = rows.sum(axis=1, dtype=np.uint64)[(r[valid] % np.uint64(2048)).astype(np.int64)].sum(dtype=np.uint64)
    assert dc.as_triples(got) == [(c[0] * e1 * e2, int(total), int(wsum))]


def test_argument_rules(eng):
    lib = eng._lib
    d, d_out = eng.alloc(4096), eng.alloc(4 * REC)
    try:
        def call(p, n, c, v, o, stream=0):
            return lib.dsx_brick_digest_u16_device(eng._ctx, ctypes.c_void_p(p), *n, *c, *v, ctypes.c_void_p(o), stream)

        one, c = (1, 1, 1), (2, 3, 5)
        assert call(d.ptr, one, c, c, d_out.ptr) == 0
        for bad in [
            (None, one, c, c, d_out.ptr), (d.ptr, one, c, c, None), (d.ptr + 1, one, c, c, d_out.ptr),
            (d.ptr, one, c, c, d_out.ptr + 4), (d.ptr, (0, 1, 1), c, c, d_out.ptr), (d.ptr, one, (2, 0, 5), c, d_out.ptr),
            (d.ptr, one, c, (2, 3, 6), d_out.ptr), (d.ptr, (1, 1, 2), (1, 3, 5), (1, 3, 5), d_out.ptr),
            (d.ptr, one, (1 << 11, 1 << 10, (1 << 10) + 1), (1, 1, 1), d_out.ptr), (d.ptr, one, c, c, d_out.ptr, 7),
        ]:  # fmt: skip
            assert call(*bad) == DSX_EINVAL, bad
        with pytest.raises(ValueError):
            eng.brick_digest(d, one, c, (2, 3, 6), d_out)
        for kw in (dict(offset=4 * REC), dict(offset=4), dict(offset=-REC)):  # records that do not fit d_out
            with pytest.raises(ValueError):
                eng.brick_digest(d, one, c, c, d_out, **kw)
        with pytest.raises(ValueError):  # more bricks than the buffer holds
            eng.brick_digest(d, (1, 1, 2), (8, 16, 16), (8, 16, 32), d_out)
        eng.sync()  # nothing was launched by the refused calls, nothing is pending
    finally:
        d.free()
        d_out.free()
