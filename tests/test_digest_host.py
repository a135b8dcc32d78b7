"""The chunk digest's host build (``dsx_brick_digest_u16_ref`` / ``engine.brick_digest_ref``; ``csrc/dsx_digest.h``)
against its NumPy uint64 restatement (``digest_cases.restate``) -- exact integers, compared for equality -- the known
answers of the contract, what a digest must and must not notice, the argument rules, and the same code built with g++
from ``tests/host/digest_check.cpp`` under ASan / UBSan as its own process.  No GPU needed."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import digest_cases as dc
from aind_smartspim_destripe_amd import engine as eng_mod

HERE = os.path.dirname(os.path.abspath(__file__))
DSX_EINVAL = -1
BRICKS, GRIDS = dc.brick_cases(), dc.grid_cases()


def test_weight_known_answers():
    assert dc.m_int(0) == 0xE220A8397B1DCDAF  # the first two outputs of splitmix64 seeded with 0
    assert dc.m_int(1) == 0x6E789E6AA1B965F5
    assert dc.m_int(1 << 32) == 0x46093CF9861EC2E5
    ks = np.array([0, 1, 1 << 32, 12345, (1 << 32) + 4103], np.uint64)
    assert [int(x) for x in dc.m_np(ks)] == [dc.m_int(int(k)) for k in ks]
    assert all(dc.m_int(k) & 1 for k in range(1000))


KNOWN = [
    ("poly", None, (30, 0xEF24, 0x0438751852D64D78)),
    ("poly", (2, 2, 4), (16, 0x57F8, 0xC504AE6B19F5C824)),
    ("ones", None, (30, 0x1DFFE2, 0x74F9A257863EB87E)),
]


@pytest.mark.parametrize("kind,extents,record", KNOWN, ids=["poly-full", "poly-2x2x4", "ones-full"])
def test_digest_known_answers(kind, extents, record):
    i = np.arange(30, dtype=np.int64)
    v = ((7 * i * i + 3 * i + 1) % 65536 if kind == "poly" else np.full(30, 65535)).astype(np.uint16).reshape(2, 3, 5)
    e = extents or (2, 3, 5)
    assert dc.restate_int(v, e) == record
    assert dc.restate(v, e) == record
    assert dc.as_triples(eng_mod.brick_digest_ref(v, (1, 1, 1), (2, 3, 5), e)) == [record]


@pytest.mark.parametrize("name,buf,first,c,e", BRICKS, ids=[b[0] for b in BRICKS])
def test_host_build_is_the_restatement(name, buf, first, c, e):
    n = int(np.prod(c))
    got = eng_mod.brick_digest_ref(buf[first : first + n], (1, 1, 1), c, e)
    assert got.dtype == eng_mod.DIGEST_DTYPE and got.shape == (1,)
    assert dc.as_triples(got) == [dc.restate(buf[first : first + n].reshape(c), e)]


@pytest.mark.parametrize("name,buf,first,c,v", GRIDS, ids=[g[0] for g in GRIDS])
def test_host_build_grids(name, buf, first, c, v):
    got = eng_mod.brick_digest_ref(buf[first:], dc.GRID, c, v)
    assert dc.as_triples(got) == dc.restate_grid(buf, first, c, v)


def test_restatement_in_python_integers():
    for c in [(1, 1, 1), (2, 3, 5), (4, 8, 16)]:
        v = dc.data("random", int(np.prod(c)), 7).reshape(c)
        for e in dc.extents_of(c):
            assert dc.restate(v, e) == dc.restate_int(v, e)


def _wsum(v, c, e):
    return int(eng_mod.brick_digest_ref(v, (1, 1, 1), c, e)["wsum"][0])


def test_any_single_voxel_change_changes_wsum():
    """Every weight m(r) * m(2^32 + i2) is odd, hence invertible mod 2^64: a change of one voxel by d, 0 < |d| < 2^16,
    moves wsum by d * (odd) != 0."""
    c = (3, 4, 11)
    v = dc.data("random", int(np.prod(c)), 9).reshape(c)
    v[0, 0, 0], v[1, 1, 1] = 0, 65535  # (so that both directions exist somewhere; the others go both ways)
    base = _wsum(v, c, c)
    for i in np.ndindex(*c):
        for d in (-1, 1):
            if 0 <= int(v[i]) + d <= 65535:
                w = v.copy()
                w[i] = int(v[i]) + d
                assert _wsum(w, c, c) != base, (i, d)
    for d in (0x8000, 0xFFFF):
        w = np.zeros(c, np.uint16)
        z = _wsum(w, c, c)
        w[2, 3, 10] = d
        assert z == 0 and _wsum(w, c, c) == (d * dc.m_int(2 * 4 + 3) * dc.m_int(dc.COL_BASE + 10)) & dc.MASK != 0


def test_swapping_two_unequal_voxels_changes_wsum():
    c = (3, 4, 11)
    v = dc.data("random", int(np.prod(c)), 10).reshape(c)
    base = eng_mod.brick_digest_ref(v, (1, 1, 1), c, c)
    flat = v.reshape(-1)
    pairs = [(0, 1), (0, 11), (0, 44), (5, 131), (130, 131), (10, 11)]  # along a row, across rows, across planes
    for a, b in pairs:
        w = flat.copy()
        assert w[a] != w[b]
        w[a], w[b] = flat[b], flat[a]
        got = eng_mod.brick_digest_ref(w, (1, 1, 1), c, c)
        assert got["sum"][0] == base["sum"][0] and got["count"][0] == base["count"][0]
        assert got["wsum"][0] != base["wsum"][0], (a, b)


def test_padding_never_enters():
    c, e = (3, 5, 130), (2, 4, 129)
    v = dc.data("random", int(np.prod(c)), 11).reshape(c)
    base = eng_mod.brick_digest_ref(v, (1, 1, 1), c, e)
    w = v.copy()
    w[2:], w[:, 4:], w[:, :, 129:] = 0x1234, 0xFFFF, 0
    assert np.array_equal(w[:2, :4, :129], v[:2, :4, :129])
    assert eng_mod.brick_digest_ref(w, (1, 1, 1), c, e) == base
    # and a voxel's weight does not depend on the extents: the valid part of a larger extent, zero elsewhere
    z = np.zeros(c, np.uint16)
    z[:2, :4, :129] = v[:2, :4, :129]
    full = eng_mod.brick_digest_ref(z, (1, 1, 1), c, c)
    assert full["wsum"][0] == base["wsum"][0] and full["sum"][0] == base["sum"][0]
    assert full["count"][0] == 3 * 5 * 130 and base["count"][0] == 2 * 4 * 129


def test_argument_rules():
    lib = eng_mod.load_library()
    vox = np.arange(2 * 3 * 5 + 1, dtype=np.uint16)
    out = np.zeros(4, np.uint64)
    vp, op = vox.ctypes.data, out.ctypes.data

    def call(p, n, c, v, o):
        return lib.dsx_brick_digest_u16_ref(ctypes.c_void_p(p), *n, *c, *v, ctypes.c_void_p(o))

    one, c = (1, 1, 1), (2, 3, 5)
    assert call(vp, one, c, c, op) == 0 and out[0] == 30
    assert call(vp + 2, one, c, c, op) == 0  # 2-byte aligned is enough
    for bad in [
        (None, one, c, c, op), (vp, one, c, c, None), (vp + 1, one, c, c, op), (vp, one, c, c, op + 4),
        (vp, (0, 1, 1), c, c, op), (vp, one, (2, 0, 5), c, op), (vp, one, c, (2, 3, 6), op), (vp, one, c, (0, 3, 5), op),
        (vp, (1, 1, 2), (1, 3, 5), (1, 3, 5), op), (vp, one, (1 << 11, 1 << 10, (1 << 10) + 1), (1, 1, 1), op),
        (vp, one, (1 << 16, 1 << 16, 1 << 16), (1, 1, 1), op),
    ]:  # fmt: skip
        assert call(*bad) == DSX_EINVAL, bad
        assert lib.dsx_last_error(None).decode().startswith("digest:")
    with pytest.raises(ValueError):
        eng_mod.brick_digest_ref(vox.astype(np.int16), one, c, c)
    with pytest.raises(ValueError):
        eng_mod.brick_digest_ref(vox[:29], one, c, c)
    with pytest.raises(ValueError):
        eng_mod.brick_digest_ref(vox, one, c, (2, 3))
    with pytest.raises(ValueError):
        eng_mod.brick_digest_ref(vox, one, c, (2, 3, 1 << 31))
    assert eng_mod.DIGEST_DTYPE.itemsize == 24 and eng_mod.DIGEST_DTYPE.names == ("count", "sum", "wsum")


def test_host_build_under_sanitizers(tmp_path):
    """tests/host/digest_check.cpp with ASan / UBSan: the weight's known answers, the launch geometry over every row
    length up to 5000, the refusals, and three ragged grids read from buffers of exactly their size."""
    exe = str(tmp_path / "digest_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "digest_check.cpp")], check=True)  # fmt: skip
    picked = [g for g in GRIDS if g[0] in ("grid-c2x3x5-short1-off1", "grid-c3x5x130-most-off0", "grid-c1x3x4104-short1-off1")]
    assert len(picked) == 3
    for name, buf, first, c, v in picked:
        raw, out = str(tmp_path / (name + ".raw")), str(tmp_path / (name + ".rec"))
        buf.tofile(raw)
        res = subprocess.run([exe, raw, str(first)] + [str(x) for x in dc.GRID + tuple(c) + tuple(v)] + [out],
                             capture_output=True, text=True)  # fmt: skip
        assert res.returncode == 0, (name, res.returncode, res.stderr[-2000:])
        got = np.fromfile(out, np.uint64).reshape(-1, 3)
        assert [tuple(int(x) for x in r) for r in got] == dc.restate_grid(buf, first, c, v), name
