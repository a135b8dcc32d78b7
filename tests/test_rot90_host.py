"""The quarter turn on the CPU: ``dsx_rot90_ref`` (the host build of the index map ``k_rot90`` uses, csrc/dsx_rot90.h)
against ``np.rot90``, and the same map together with the launch geometry through tests/host/dsx_rot90_check.cpp, built
with g++ once plain and once with the address and undefined-behaviour sanitizers.  No GPU needed."""

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "dsx_rot90_check.cpp")
SHAPES = [(1, 1), (1, 7), (3, 5), (63, 65), (64, 64), (70, 100), (129, 257)]
CANARY = 64  # bytes either side of the destination


def _planes(dtype, n, H, W):
    rng = np.random.default_rng(H * 1000 + W + n)
    if dtype == np.uint16:
        return rng.integers(0, 65536, (n, H, W), dtype=np.uint16)
    return rng.standard_normal((n, H, W)).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_rot90_ref_is_np_rot90(shape, dtype):
    lib = engine.load_library()
    H, W = shape
    for n in (1, 3):
        x = _planes(dtype, n, H, W)
        for direction in (1, -1):
            nbytes = x.nbytes
            raw = np.full(nbytes + 2 * CANARY, 0xA5, np.uint8)
            dst = raw[CANARY : CANARY + nbytes]
            rc = lib.dsx_rot90_ref(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dst.ctypes.data),
                                   engine._dtype_code(dtype), n, H, W, direction)  # fmt: skip
            assert rc == 0
            got = dst.view(dtype).reshape(n, W, H)
            np.testing.assert_array_equal(got, np.rot90(x, direction, axes=(1, 2)))
            assert (raw[:CANARY] == 0xA5).all() and (raw[CANARY + nbytes :] == 0xA5).all()
        np.testing.assert_array_equal(engine.rot90_ref(x, 1), np.rot90(x, 1, axes=(1, 2)))


def test_rot90_ref_refuses_bad_arguments():
    lib = engine.load_library()
    a = np.zeros((2, 3), np.uint16)
    b = np.zeros((3, 2), np.uint16)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.dsx_rot90_ref(p(a), p(b), engine.DSX_U16, 1, 2, 3, 0) == -1  # dir
    assert lib.dsx_rot90_ref(p(a), p(b), 7, 1, 2, 3, 1) == -1  # dtype
    assert lib.dsx_rot90_ref(p(a), p(b), engine.DSX_U16, 1, 0, 3, 1) == -1  # empty plane
    assert lib.dsx_rot90_ref(p(a), p(a), engine.DSX_U16, 1, 2, 3, 1) == -1  # in place
    assert lib.dsx_rot90_ref(None, p(b), engine.DSX_U16, 1, 2, 3, 1) == -1
    assert lib.dsx_rot90_ref(None, None, engine.DSX_U16, 0, 2, 3, 1) == 0  # nothing to do
    with pytest.raises(ValueError):
        engine.rot90_ref(np.zeros((1, 2, 3), np.uint16), 2)


def _build(path, sanitize):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", path, SRC], check=True)
    return path


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_tiles_write_every_element_once(tmp_path, sanitize):
    """Every destination element of every shape is written exactly once by the blocks of the launch grid, from the
    element ``np.rot90`` names; partial tiles at both edges are covered; the transposed LDS read touches 32 banks per
    32-lane group for both element sizes (tests/host/dsx_rot90_check.cpp)."""
    exe = _build(str(tmp_path / "dsx_rot90_check"), sanitize)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert out["ok"] and out["checked"] > 500_000, out
