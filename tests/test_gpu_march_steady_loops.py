"""The march kernels' steady loops issue loads and stores that they do not use: rows past the end of a block or a plane are
loaded from clamped addresses, and the result store of k_rowfinal is issued by every lane in every step and DISCARDED
through its buffer descriptor where a lane or a row has nothing to write (csrc/dsx_kernels.h: rowfinal_synth,
STEADY).  What must hold whatever the loops issue:

* a plane of a batch comes out bit for bit as the same plane run alone;
* every plane passes the parity statement of tests/parity_util.py against the oracle;
* nothing is written outside the result: the result buffer sits between two guard regions of 1 MiB each, filled with a
  pattern, and both are intact after the call.

Heights: 2, 4, 6, 26, 28, 30, 54, 58, 64, 200 rows -- the last k_rowfinal block of a 2048-wide plane then holds 1, 2, 3, 13,
14, 1, 13, 1, 4 and 2 coefficient rows (a block holds 14), so the loop is left after every one of its three row pairs,
with and without a second row in the last pair, in its first trip and in a later one.  2000- and 1800-wide planes take the
fused final k_inv_march instead, 72 x 136 and 50 x 70 planes the coarse kernels alone, float32 results the unfused final
kernel.
"""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import synth
from parity_util import check_plane, gpu_deltas, oracle_plane

pytestmark = pytest.mark.gpu

GUARD = 1 << 20  # bytes in front of and behind the result
HEIGHTS = (2, 4, 6, 26, 28, 30, 54, 58, 64, 200)
MAX_FLIPS = lambda size: max(3, int(2e-5 * size))  # noqa: E731  (tests/test_gpu_parity.py)


class _At:
    """A device address inside an allocation, for DestripeEngine.run_device."""

    def __init__(self, buf, offset):
        self.ptr = buf.ptr + offset


@pytest.fixture(scope="module")
def parity_engine():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _guard_pattern():
    return ((np.arange(GUARD, dtype=np.uint32) * 2654435761) >> 24).astype(np.uint8)


def _shading(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    flat = (1.0 - 0.15 * (((yy - h / 2.0) / max(h / 2.0, 1.0)) ** 2 + ((xx - w / 2.0) / (w / 2.0)) ** 2)).astype(np.float32)
    return flat, np.full((h, w), 100.0, np.float32)


class _Guarded:
    """An engine planned for one shape whose results land between two guard regions."""

    def __init__(self, h, w, n_max, out_dtype, shading=False):
        self.h, self.w, self.out_dtype = h, w, np.dtype(out_dtype)
        self.flat, self.dark = _shading(h, w) if shading else (None, None)
        self.e = eng_mod.DestripeEngine(0)
        self.e.plan(h, w, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=n_max,
                    flatfield=self.flat, darkfield=self.dark)  # fmt: skip
        assert self.e.out_shape == (h, w)
        self.pattern = _guard_pattern()
        self.d_in = self.e.alloc(n_max * h * w * 2)
        self.d_out = self.e.alloc(2 * GUARD + n_max * h * w * self.out_dtype.itemsize)

    def run(self, planes):
        n = planes.shape[0]
        nbytes = n * self.h * self.w * self.out_dtype.itemsize
        self.d_in.upload(planes)
        self.d_out.upload(self.pattern, 0)
        self.d_out.upload(self.pattern, GUARD + nbytes)
        self.e.run_device(self.d_in, np.uint16, n, _At(self.d_out, GUARD), self.out_dtype.type)
        self.e.sync()
        front = self.d_out.download((GUARD,), np.uint8, 0)
        back = self.d_out.download((GUARD,), np.uint8, GUARD + nbytes)
        assert np.array_equal(front, self.pattern), ("written in front of the result", int((front != self.pattern).sum()))
        assert np.array_equal(back, self.pattern), ("written behind the result", int((back != self.pattern).sum()))
        return self.d_out.download((n, self.h, self.w), self.out_dtype.type, GUARD)

    def close(self):
        self.d_in.free()
        self.d_out.free()
        self.e.close()


_ALONE = {}  # (h, w, out dtype, shading) -> (planes, each plane's result run alone): computed once, shared, not modified


def _alone(h, w, out_dtype, shading, n):
    key = (h, w, np.dtype(out_dtype).name, shading)
    if key not in _ALONE or len(_ALONE[key][1]) < n:
        planes = synth.synthetic_bank(5, h, w)
        g = _Guarded(h, w, 1, out_dtype, shading)
        try:
            res = [g.run(planes[k : k + 1])[0] for k in range(n)]
        finally:
            g.close()
        _ALONE[key] = (planes, res)
    return _ALONE[key]


def _batch_is_the_planes_alone(h, w, n, out_dtype=np.uint16, shading=False):
    planes, alone = _alone(h, w, out_dtype, shading, n)
    if n > 1:
        g = _Guarded(h, w, n, out_dtype, shading)
        try:
            got = g.run(planes[:n])
        finally:
            g.close()
        for k in range(n):
            np.testing.assert_array_equal(got[k], alone[k], err_msg=str((h, w, n, k, "batch against the plane alone")))
    return planes, alone


_PROVEN = set()


def _u16_parity(engine, h, w, n, planes, alone, shading=False):
    """check_plane for stored uint16 planes, as parity_util.u16_plane_parity states it: the plane's float32 result passes
    check_plane against the oracle, and every stored value is that result (through the reference's dark / flat
    arithmetic in float64 with shading) truncated, within one count.  Written out here because planes of 2, 4 and 6 rows
    have no decomposition level: both configs then compute the same thing and the engine does not evaluate the
    foreground statistic that would choose between them, so the config index is compared only where a level exists."""
    for k in range(n):
        if (h, w, shading, k) in _PROVEN:  # the same plane and the same bits as in the case that proved it
            continue
        what = "{}x{} plane {}{}".format(h, w, k, " shading" if shading else "")
        deltas = gpu_deltas(engine, planes[k : k + 1])
        f32, cfg = engine.run(planes[k : k + 1], out_dtype=np.float32, return_cfg=True)
        which, _, _, ref, stages = oracle_plane(planes[k])
        if stages:
            assert int(cfg[0]) == which, (what, int(cfg[0]), which)
        cfgd = synth.CELLS_CONFIG if which else synth.NO_CELLS_CONFIG
        n_bad, flips = check_plane(f32[0], planes[k], deltas[0], what, cfgd, MAX_FLIPS, ref=ref, stages=stages)
        x = f32[0].astype(np.float64)
        if shading:
            flat, dark = _shading(h, w)
            x = np.where(x > dark, x - dark.astype(np.float64), 0.0) / flat.astype(np.float64)
        want = np.clip(x, 0, 65535).astype(np.uint16).astype(np.int64)
        d = np.abs(alone[k].astype(np.int64) - want)
        print("[steady loops] {}: flips {}, beyond 1e-4 unforced {}, one count off {:.2e}, worst {}".format(
            what, flips, n_bad, float((d > 0).mean()), int(d.max())))
        assert int(d.max()) <= 1, (what, "stored value more than one count from the float32 result", int(d.max()), int((d > 1).sum()))
        _PROVEN.add((h, w, shading, k))


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h", HEIGHTS)
def test_rowfinal_2048_wide(parity_engine, h, n):
    """uint16 planes 2048 wide: the level-1 row filter and the final synthesis in k_rowfinal."""
    planes, alone = _batch_is_the_planes_alone(h, 2048, n)
    _u16_parity(parity_engine, h, 2048, n, planes, alone)


@pytest.mark.parametrize("w", [2000, 1800])
@pytest.mark.parametrize("h", HEIGHTS)
def test_fused_final_kernel_2000_and_1800_wide(parity_engine, h, w):
    """uint16 planes 2000 and 1800 wide: k_rowfilter and the fused final k_inv_march."""
    planes, alone = _batch_is_the_planes_alone(h, w, 3)
    _u16_parity(parity_engine, h, w, 3, planes, alone)


@pytest.mark.parametrize("shape", [(72, 136), (50, 70)])
def test_coarse_kernels_only(parity_engine, shape):
    """Planes too small for anything fused: the generic and coarse march kernels on every level."""
    h, w = shape
    planes, alone = _batch_is_the_planes_alone(h, w, 3)
    _u16_parity(parity_engine, h, w, 3, planes, alone)


def test_float32_result_64_by_2048(parity_engine):
    """float32 results leave through the final k_inv_march (no k_rowfinal): check_plane on the result itself."""
    h, w, n = 64, 2048, 3
    planes, alone = _batch_is_the_planes_alone(h, w, n, out_dtype=np.float32)
    deltas = gpu_deltas(parity_engine, planes[:n])
    for k in range(n):
        which, _, _, ref, stages = oracle_plane(planes[k])
        cfg = synth.CELLS_CONFIG if which else synth.NO_CELLS_CONFIG
        check_plane(alone[k], planes[k], deltas[k], "64x2048 float32 plane {}".format(k), cfg, MAX_FLIPS, ref=ref, stages=stages)


def test_rowfinal_with_shading(parity_engine):
    """Once with the dark / flat epilogue: 58 rows (two full blocks and one coefficient row), five planes."""
    h, w, n = 58, 2048, 5
    planes, alone = _batch_is_the_planes_alone(h, w, n, shading=True)
    _u16_parity(parity_engine, h, w, n, planes, alone, shading=True)
