"""The voxel histogram's host build (``dsx_volhist_ref`` / ``engine.volhist_ref``; ``csrc/dsx_volhist.h``) against
``np.bincount``, its argument rules, and the same code built with g++ from ``tests/host/volhist_check.cpp`` under
ASan / UBSan as its own process.  No GPU needed."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import volhist_cases as vc
from aind_smartspim_destripe_amd import engine as eng_mod

HERE = os.path.dirname(os.path.abspath(__file__))
DSX_EINVAL = -1


@pytest.mark.parametrize("name,buf,start,count", vc.cases(), ids=[c[0] for c in vc.cases()])
def test_volhist_ref_is_bincount(name, buf, start, count):
    got = eng_mod.volhist_ref(buf.reshape(-1)[start : start + count])
    assert got.dtype == np.int64 and got.shape == (vc.BINS,)
    assert np.array_equal(got, vc.expected(buf, start, count))
    assert int(got.sum()) == count


def test_volhist_ref_accumulates_over_calls():
    a, b = vc.odd_random(), vc.window_edges()
    h = eng_mod.volhist_ref(a)
    assert eng_mod.volhist_ref(b, hist=h) is h
    assert np.array_equal(h, vc.expected(a, 0, a.size) + vc.expected(b, 0, b.size))
    assert np.array_equal(eng_mod.volhist_ref(np.zeros(0, np.uint16), hist=h), h)  # n == 0 adds nothing


def test_volhist_ref_argument_rules():
    lib = eng_mod.load_library()
    hist = np.zeros(vc.BINS, np.uint64)
    vox = np.arange(16, dtype=np.uint16)
    hp, vp = hist.ctypes.data_as(ctypes.c_void_p), vox.ctypes.data_as(ctypes.c_void_p)
    assert lib.dsx_volhist_ref(None, 0, hp) == 0  # n == 0 is a no-op, whatever the pointers
    assert lib.dsx_volhist_ref(None, 0, None) == 0
    assert lib.dsx_volhist_ref(None, 16, hp) == DSX_EINVAL
    assert lib.dsx_volhist_ref(vp, 16, None) == DSX_EINVAL
    assert not hist.any()
    assert lib.dsx_volhist_ref(vp, 16, hp) == 0 and int(hist.sum()) == 16
    with pytest.raises(ValueError):
        eng_mod.volhist_ref(np.zeros(4, np.int16))
    with pytest.raises(ValueError):
        eng_mod.volhist_ref(vox, hist=np.zeros(vc.BINS, np.int32))
    with pytest.raises(ValueError):
        eng_mod.volhist_ref(vox, hist=np.zeros(vc.BINS - 1, np.int64))


def test_volhist_host_build_under_sanitizers(tmp_path):
    """tests/host/volhist_check.cpp with ASan / UBSan on cases (a) and (b) and on the sub-range of (e): the counts, and
    no read outside the range or count outside the 65 536 bins."""
    exe = str(tmp_path / "volhist_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "volhist_check.cpp")], check=True)  # fmt: skip
    for name, buf, start, count in vc.cases():
        if name[0] not in "abe":
            continue
        raw, out = str(tmp_path / (name + ".raw")), str(tmp_path / (name + ".hist"))
        buf.tofile(raw)
        res = subprocess.run([exe, raw, str(start), str(count), out], capture_output=True, text=True)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        assert np.array_equal(np.fromfile(out, np.uint64).astype(np.int64), vc.expected(buf, start, count)), name
