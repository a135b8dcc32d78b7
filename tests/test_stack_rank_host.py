"""The stack-rank kernel's host build (``dsx_stack_rank_u16_ref`` / ``engine.stack_rank_ref``; ``csrc/dsx_stackrank.h``)
against the contract restated in NumPy, its argument rules, the launch geometry, and the same code built with g++ from
``tests/host/stack_rank_check.cpp`` under ASan / UBSan as its own process.  No GPU needed."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import stack_rank_cases as sc
from aind_smartspim_destripe_amd import engine as eng_mod

HERE = os.path.dirname(os.path.abspath(__file__))
DSX_EINVAL = -1


@pytest.mark.parametrize("case", sc.cases(), ids=sc.ids())
def test_stack_rank_ref_is_the_contract(case):
    before = case.stack.copy()
    out, valid = eng_mod.stack_rank_ref(case.stack, case.q_milli, (case.lo, case.hi))
    want_out, want_valid = sc.expected(case)
    assert out.dtype == np.uint16 and out.shape == want_out.shape
    assert valid.dtype == np.uint16 and valid.shape == want_valid.shape
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(out, want_out)
    assert np.array_equal(case.stack, before)


def test_the_cases_cover_what_they_claim():
    by = {c.name: c for c in sc.cases()}
    assert by["guarded_n128_p2048"].stack.ctypes.data % 16 == 2 and by["vec_n128_p2048"].stack.ctypes.data % 16 == 0
    for name in ("window_sparse_n3", "window_sparse_n257"):
        valid = sc.expected(by[name])[1]
        assert set(np.unique(valid)) == {0, 1}
    assert by["ranks_n512_p257"].stack.max() >= 0x8000
    want = sc.expected(by["ranks_n512_p257"])[0]
    assert np.all(want[0] == 0) and np.all(want[1] == 128 * 255) and np.all(want[3] == 128 * 511)
    # one of the pairs where NumPy's float rule (method="lower") takes another rank
    assert int(np.floor(290 / 1000 * (101 - 1))) == 28 and sc.rank_of(290, 101) == 29
    differ = sum(int(np.floor(q / 1000 * (m - 1))) != sc.rank_of(q, m) for m in range(1, 513) for q in range(1001))
    assert differ == 41
    c = by["float_rule_m101_q290"]
    col = np.sort(c.stack, axis=0)
    assert np.array_equal(sc.expected(c)[0][0], col[29]) and not np.array_equal(col[28], col[29])


def _call(lib, stack, n, P, lo, hi, q, out, valid):
    qa = (ctypes.c_int * max(len(q), 1))(*q)
    vp = ctypes.c_void_p
    return lib.dsx_stack_rank_u16_ref(None if stack is None else stack.ctypes.data_as(vp), n, P, lo, hi, qa, len(q),
                                      None if out is None else out.ctypes.data_as(vp),
                                      None if valid is None else valid.ctypes.data_as(vp))  # fmt: skip


def test_stack_rank_ref_argument_rules():
    lib = eng_mod.load_library()
    stack = np.arange(3 * 8, dtype=np.uint16).reshape(3, 8)
    out = np.full((4, 8), 7, np.uint16)
    valid = np.full(8, 7, np.uint16)
    ok = dict(stack=stack, n=3, P=8, lo=0, hi=65535, q=[500], out=out, valid=valid)
    bad = [dict(n=0), dict(n=513), dict(n=-1), dict(q=[]), dict(q=[1, 2, 3, 4, 5]), dict(P=0), dict(P=1 << 31),
           dict(lo=-1), dict(hi=65536), dict(lo=5, hi=4), dict(q=[-1]), dict(q=[1001]), dict(q=[500, 1001]),
           dict(stack=None), dict(out=None)]  # fmt: skip
    for change in bad:
        assert _call(lib, **dict(ok, **change)) == DSX_EINVAL, change
    assert np.all(out == 7) and np.all(valid == 7)  # nothing was written
    assert _call(lib, **dict(ok, valid=None)) == 0  # valid may be NULL
    assert np.array_equal(out[0], stack[1]) and np.all(valid == 7)
    assert _call(lib, **dict(ok, n=512, P=(1 << 31) - 1, stack=None)) == DSX_EINVAL  # the limits themselves pass the
    assert b"NULL" in lib.dsx_last_error(None)  # range checks: what is refused here is the pointer

    for kwargs in (dict(q_milli=[]), dict(q_milli=[1, 2, 3, 4, 5]), dict(q_milli=[1001]), dict(q_milli=[0.5]),
                   dict(q_milli=500), dict(valid_range=(5, 4)), dict(valid_range=(-1, 4)), dict(valid_range=(0, 65536)),
                   dict(valid_range=(0,)), dict(valid_range=(0.0, 10.0))):  # fmt: skip
        with pytest.raises(ValueError):
            eng_mod.stack_rank_ref(stack, **dict(dict(q_milli=[500], valid_range=(0, 65535)), **kwargs))
    with pytest.raises(ValueError):
        eng_mod.stack_rank_ref(stack.astype(np.int16), [500])
    with pytest.raises(ValueError):
        eng_mod.stack_rank_ref(np.zeros((513, 4), np.uint16), [500])
    with pytest.raises(ValueError):
        eng_mod.stack_rank_ref(np.zeros(4, np.uint16), [500])
    with pytest.raises(ValueError):
        eng_mod.stack_rank_args(513, 4, [500], (0, 65535))
    with pytest.raises(ValueError):
        eng_mod.stack_rank_args(4, 1 << 31, [500], (0, 65535))
    assert eng_mod.stack_rank_args(512, (1 << 31) - 1, (0, 1000, 5, 5), (0, 65535)) == (512, (1 << 31) - 1, [0, 1000, 5, 5], 0, 65535)


def test_stack_rank_ref_keeps_plane_shape():
    stack = sc.cases()[0].stack[:, : 37 * 53].reshape(-1, 37, 53)
    out, valid = eng_mod.stack_rank_ref(stack, (500,))
    assert out.shape == (1, 37, 53) and valid.shape == (37, 53)
    assert np.array_equal(out.reshape(1, -1), sc.expected(sc.cases()[0])[0][1:2])


def test_stack_rank_host_build_under_sanitizers(tmp_path):
    """tests/host/stack_rank_check.cpp with ASan / UBSan on three cases: the result, no access outside the stack or the
    results, and the launch geometry over every n (the program returns 4 when a tile would not fit or cover)."""
    exe = str(tmp_path / "stack_rank_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "stack_rank_check.cpp")], check=True)  # fmt: skip
    picked = [c for c in sc.cases() if c.name in ("noise_n257_p1961", "guarded_n128_p2048", "window_sparse_n3")]
    assert len(picked) == 3
    for c in picked:
        n, P = c.stack.shape
        raw, res = str(tmp_path / (c.name + ".raw")), str(tmp_path / (c.name + ".out"))
        whole = c.stack.base if c.lead else c.stack
        np.asarray(whole).reshape(-1).tofile(raw)
        q = list(c.q_milli) + [0] * (4 - len(c.q_milli))
        args = [exe, raw, c.lead, n, P, c.lo, c.hi, len(c.q_milli)] + q + [res]
        run = subprocess.run([str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, (c.name, run.returncode, run.stderr[-2000:])
        got = np.fromfile(res, np.uint16)
        want_out, want_valid = sc.expected(c)
        assert np.array_equal(got[: want_out.size].reshape(want_out.shape), want_out), c.name
        assert np.array_equal(got[want_out.size :], want_valid), c.name
