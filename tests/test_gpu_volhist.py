"""``k_volhist_u16`` (``csrc/dsx_volhist.h``) on the device against its host build, exactly: window edges, odd sizes,
worst-case contention inside and outside the LDS window, accumulation / reset, unaligned sub-ranges, arguments."""

import ctypes

import numpy as np
import pytest

import volhist_cases as vc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu

DSX_EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reference():
    """The host build's counts of every case, computed once."""
    return {name: eng_mod.volhist_ref(buf.reshape(-1)[start : start + count]) for name, buf, start, count in vc.cases()}


def _device_hist(e, buf, start, count):
    d = e.alloc(max(buf.nbytes, 16))
    try:
        d.upload(buf)
        e.volhist_reset()
        e.volhist_add(d.ptr + 2 * start, count)
        return e.volhist_get()
    finally:
        d.free()


@pytest.mark.parametrize("name,buf,start,count", vc.cases(), ids=[c[0] for c in vc.cases()])
def test_device_histogram_is_the_host_build(eng, reference, name, buf, start, count):
    if name.startswith("e_"):
        assert (2 * start) % 16 == 2  # 2-byte aligned only (device allocations are 256-byte aligned)
    got = _device_hist(eng, buf, start, count)
    assert got.dtype == np.int64 and got.shape == (vc.BINS,)
    assert int(got.sum()) == count
    assert np.array_equal(got, reference[name])
    if name.startswith("e_"):
        assert got[vc.SENTINEL] == 0  # nothing on either side of the range was counted


def test_every_head_and_tail_length(eng):
    """Ranges that start 0 .. 8 voxels past a 16-byte boundary and end 0 .. 8 voxels past a whole vector, short enough
    to have no vector at all and long enough to have some."""
    g = vc.guarded().reshape(-1)
    plane = vc.ODD[1] * vc.ODD[2]
    d = eng.alloc(g.nbytes)
    try:
        d.upload(g)
        for start in range(plane, plane + 9):
            for count in (1, 5, 7, 8, 9, 23, 64, 65, 1024 + 3):
                eng.volhist_reset()
                eng.volhist_add(d.ptr + 2 * start, count)
                assert np.array_equal(eng.volhist_get(), vc.expected(g, start, count)), (start, count)
    finally:
        d.free()


def test_accumulation_reset_and_two_engines(eng, reference):
    a, b = vc.odd_random(), vc.constant(150)
    other = eng_mod.DestripeEngine(0)
    da, db = eng.alloc(a.nbytes), eng.alloc(b.nbytes)
    do = other.alloc(a.nbytes)
    try:
        da.upload(a)
        db.upload(b)
        do.upload(a)
        eng.volhist_reset()
        other.volhist_reset()
        eng.volhist_add(da, a.size)
        eng.volhist_add(db, b.size)
        other.volhist_add(do, a.size)
        both = eng.volhist_get()
        assert np.array_equal(both, reference["b_odd_sizes"] + reference["c_constant_150"])
        assert np.array_equal(other.volhist_get(), reference["b_odd_sizes"])  # its own buffer
        assert np.array_equal(eng.volhist_get(), both)  # reading does not clear
        eng.volhist_reset()
        assert not eng.volhist_get().any()
        assert np.array_equal(other.volhist_get(), reference["b_odd_sizes"])
    finally:
        for d in (da, db, do):
            d.free()
        other.close()


def test_histogram_survives_a_plan_change(eng, reference):
    from aind_smartspim_destripe_amd import synth

    a = vc.odd_random()
    d = eng.alloc(a.nbytes)
    try:
        d.upload(a)
        eng.volhist_reset()
        eng.volhist_add(d, a.size)
        eng.plan(64, 64, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, max_batch=2)
        eng.volhist_add(d, a.size)
        assert np.array_equal(eng.volhist_get(), 2 * reference["b_odd_sizes"])
    finally:
        d.free()


def test_arguments():
    e = eng_mod.DestripeEngine(0)
    lib, ctx = e._lib, e._ctx
    d = e.alloc(64)
    hist = np.zeros(vc.BINS, np.uint64)
    hp = hist.ctypes.data_as(ctypes.c_void_p)
    try:
        d.upload(np.full(32, 7, np.uint16))
        assert lib.dsx_volhist_add_device(ctx, ctypes.c_void_p(d.ptr), 32) == DSX_EINVAL  # before the first reset
        assert lib.dsx_volhist_get(ctx, hp) == DSX_EINVAL
        with pytest.raises(eng_mod.DsxError):
            e.volhist_get()
        e.volhist_reset()
        assert lib.dsx_volhist_add_device(ctx, ctypes.c_void_p(d.ptr), 0) == 0  # no-op
        assert lib.dsx_volhist_add_device(ctx, None, 0) == 0
        assert lib.dsx_volhist_add_device(ctx, None, 32) == DSX_EINVAL
        assert lib.dsx_volhist_get(ctx, None) == DSX_EINVAL
        assert lib.dsx_volhist_add_device(ctx, ctypes.c_void_p(d.ptr), 1 << 32) == -5  # DSX_ELIMIT, nothing launched
        assert not e.volhist_get().any()
        e.volhist_add(d, 32)
        got = e.volhist_get()
        assert got[7] == 32 and got.sum() == 32
    finally:
        d.free()
        e.close()
