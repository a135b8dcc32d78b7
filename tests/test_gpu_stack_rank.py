"""``k_stack_rank_u16`` (``csrc/dsx_stackrank.h``) on the device against its host build, exactly: both sides of every
tile-width switch, odd and ragged plane sizes, the 16-byte and the 2-byte load body, values at and above 0x8000, windows
that empty pixels, several quantiles per call, sentinels around the results, arguments."""

import ctypes

import numpy as np
import pytest

import stack_rank_cases as sc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu

DSX_EINVAL = -1
GUARD = 0xABCD


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reference():
    """The host build's results of every case, computed once."""
    return {c.name: eng_mod.stack_rank_ref(c.stack, c.q_milli, (c.lo, c.hi)) for c in sc.cases()}


def _guarded_buffer(e, elems):
    """A device buffer of ``elems`` uint16 with one guard element on either side, all set to GUARD."""
    d = e.alloc(2 * (elems + 2))
    d.upload(np.full(elems + 2, GUARD, np.uint16))
    return d


def _device_rank(e, whole, lead, n, P, q, window, want_valid=True):
    """Runs the kernel on ``n`` planes of ``P`` elements that start ``lead`` elements into the flat uint16 array
    ``whole``; results go one element into guarded buffers.  Returns ``(out [n_q, P], valid [P] or None)`` after checking
    that the guards and the input are untouched."""
    d_in = e.alloc(max(whole.nbytes, 16))
    d_out, d_valid = _guarded_buffer(e, len(q) * P), _guarded_buffer(e, P)
    try:
        d_in.upload(whole)
        if want_valid:
            e.stack_rank(d_in.ptr + 2 * lead, n, P, q, window, d_out=d_out.ptr + 2, d_valid=d_valid.ptr + 2)
        else:
            rc = e._lib.dsx_stack_rank_u16_device(e._ctx, ctypes.c_void_p(d_in.ptr + 2 * lead), n, P, window[0], window[1],
                                                  (ctypes.c_int * len(q))(*q), len(q), ctypes.c_void_p(d_out.ptr + 2),
                                                  None)  # fmt: skip
            assert rc == 0
        e.sync()
        out = d_out.download(len(q) * P + 2, np.uint16)
        valid = d_valid.download(P + 2, np.uint16)
        assert out[0] == GUARD and out[-1] == GUARD
        assert valid[0] == GUARD and valid[-1] == GUARD
        if not want_valid:
            assert np.all(valid == GUARD)
        assert np.array_equal(d_in.download(whole.shape, np.uint16), whole)
        return out[1:-1].reshape(len(q), P), valid[1:-1] if want_valid else None
    finally:
        for d in (d_in, d_out, d_valid):
            d.free()


@pytest.mark.parametrize("case", sc.cases(), ids=sc.ids())
def test_device_rank_is_the_host_build(eng, reference, case):
    n, P = case.stack.shape
    whole = np.asarray(case.stack.base if case.lead else case.stack).reshape(-1)
    assert whole.size == n * P + 2 * case.lead
    out, valid = _device_rank(eng, whole, case.lead, n, P, case.q_milli, (case.lo, case.hi))
    want_out, want_valid = reference[case.name]
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(out, want_out)


def test_sub_range_of_a_stack_and_no_valid_plane(eng):
    """Planes 1 .. 129 of a 131-plane stack of odd planes (``d.ptr + 2 * P``: 2-byte aligned only), with guard planes
    of another value range on either side, and the call without a ``valid`` plane."""
    P, n = 37 * 53, 129
    rs = np.random.RandomState(31)
    whole = np.full((n + 2, P), 60000, np.uint16)
    whole[1:-1] = rs.randint(0, 30000, (n, P))
    want_out, want_valid = eng_mod.stack_rank_ref(whole[1:-1], (0, 500, 1000))
    assert want_out.max() < 30000
    out, valid = _device_rank(eng, whole.reshape(-1), P, n, P, (0, 500, 1000), (0, 65535))
    assert np.array_equal(out, want_out) and np.array_equal(valid, want_valid)
    out, valid = _device_rank(eng, whole.reshape(-1), P, n, P, (0, 500, 1000), (0, 65535), want_valid=False)
    assert np.array_equal(out, want_out) and valid is None


def test_buffers_are_allocated_when_not_given(eng):
    c = {c.name: c for c in sc.cases()}["noise_n129_p35"]
    d = eng.alloc(c.stack.nbytes)
    try:
        d.upload(c.stack)
        d_out, d_valid = eng.stack_rank(d, 129, 35, c.q_milli)
        eng.sync()
        want_out, want_valid = sc.expected(c)
        assert np.array_equal(d_out.download(want_out.shape, np.uint16), want_out)
        assert np.array_equal(d_valid.download(want_valid.shape, np.uint16), want_valid)
        d_out.free()
        d_valid.free()
    finally:
        d.free()


def test_arguments_are_refused_with_no_launch(eng):
    lib, ctx = eng._lib, eng._ctx
    P = 64
    d_in = eng.alloc(2 * 513 * P)
    d_out, d_valid = _guarded_buffer(eng, 4 * P), _guarded_buffer(eng, P)
    vp = ctypes.c_void_p
    try:
        d_in.upload(np.zeros(513 * P, np.uint16))

        def call(n=3, P=P, lo=0, hi=65535, q=(500,), planes=d_in.ptr, out=d_out.ptr + 2, valid=d_valid.ptr + 2):
            return lib.dsx_stack_rank_u16_device(ctx, vp(planes) if planes else None, n, P, lo, hi,
                                                 (ctypes.c_int * max(len(q), 1))(*q), len(q),
                                                 vp(out) if out else None, vp(valid) if valid else None)  # fmt: skip

        for change in (dict(n=513), dict(q=(1, 2, 3, 4, 5)), dict(n=0), dict(q=()), dict(P=0), dict(P=1 << 31),
                       dict(lo=-1), dict(hi=65536), dict(lo=9, hi=8), dict(q=(1001,)), dict(q=(-1,)), dict(planes=0),
                       dict(out=0), dict(planes=d_in.ptr + 1)):  # fmt: skip
            assert call(**change) == DSX_EINVAL, change
        assert lib.dsx_stack_rank_u16_device(None, vp(d_in.ptr), 3, P, 0, 65535, (ctypes.c_int * 1)(500), 1,
                                             vp(d_out.ptr + 2), None) == DSX_EINVAL  # fmt: skip
        with pytest.raises(ValueError):
            eng.stack_rank(d_in, 513, P, (500,), d_out=d_out.ptr + 2, d_valid=d_valid.ptr + 2)
        with pytest.raises(ValueError):
            eng.stack_rank(d_in, 3, P, (1, 2, 3, 4, 5), d_out=d_out.ptr + 2, d_valid=d_valid.ptr + 2)
        eng.sync()
        assert np.all(d_out.download(4 * P + 2, np.uint16) == GUARD)  # nothing ran
        assert np.all(d_valid.download(P + 2, np.uint16) == GUARD)
        assert call() == 0
        eng.sync()
        assert np.all(d_out.download(4 * P + 2, np.uint16)[1 : P + 1] == 0)
        assert np.all(d_valid.download(P + 2, np.uint16)[1:-1] == 3)
    finally:
        for d in (d_in, d_out, d_valid):
            d.free()
