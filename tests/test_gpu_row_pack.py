"""The packed coarse row filter (k_rowfilter_pack: a wave owns several row pairs of a short level and runs the median
loop and every FFT pass over them jointly) against the chain with one pair per wave (DSX_NO_ROW_PACK=1:
k_rowfilter_multi), bit for bit.

uint16 planes of 130 x 516 are the smallest that carry the coarse row shapes of the flagship's 2048^2 planes: levels of
67 x 260, 36 x 132, 20 x 68 (embedded in 144) and 12 x 36 coefficients -- direct and embedded rows, one 256-value group
plus a tail slot and tail slots only, 34 row pairs on level 1 of which the last has no partner row and, at three pairs per
wave, stands alone in its wave, and 6 pairs on the last level, which leave a wave with 2 of 4.

Planes this small never fill the chip, and a launch that does not keeps one pair per wave by default
(dsx::row_pack_runs), so besides the default context the test runs two that pack whatever the size: DSX_ROW_PACK_FILL=0
(the pack factors the benchmark runs with: 3 at M = 260, else 4), and the same with DSX_ROW_PACK=4 (4 everywhere).

How the test knows which kernel ran: the context counts its k_rowfilter_pack launches (dsx_row_pack_launches).  The
packing contexts must have enqueued one per cohort part, the context with DSX_NO_ROW_PACK=1 none; what decides between
the kernels is pinned on the CPU by tests/test_row_pack_host.py."""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import synth
from oracle import destripe_oracle as orc

pytestmark = pytest.mark.gpu

H, W, N = 130, 516, 64
SWITCHES = ("DSX_NO_ROW_PACK", "DSX_ROW_PACK", "DSX_ROW_PACK_FILL", "DSX_ROW_PACK_WPB")


@pytest.fixture(scope="module")
def stack():
    bank = synth.synthetic_bank(6, H, W)  # planes 0 and 4 carry cells: both config outcomes
    flat = np.full((H, W), 300, np.uint16)  # no coefficient above a threshold: the median is skipped for whole waves
    rows = np.repeat((100 + 50 * np.arange(H, dtype=np.uint16) % 7)[:, None], W, axis=1).astype(np.uint16)  # constant rows
    s = np.concatenate([bank, flat[None], rows[None], synth.synthetic_stack(N - 8, H, W, bank=bank)])
    s.setflags(write=False)
    return s


def _run(monkeypatch, stack, cells_cfg, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = eng_mod.DestripeEngine(0)
    try:
        e.plan(H, W, cells_cfg, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=N)
        assert [e.level_shape(lv) for lv in range(e.levels)] == [(67, 260), (36, 132), (20, 68), (12, 36)]
        small = e.run(stack[:8], out_dtype=np.uint16)  # a small cohort that runs alone (levels 3, 4 share the launch)
        n_small = e.row_pack_launches()
        big, cfg = e.run(stack, out_dtype=np.uint16, return_cfg=True)  # 4 parts of 16 planes, all four levels in the launch
        n_big = e.row_pack_launches() - n_small
        return np.asarray(small), np.asarray(big), np.asarray(cfg), (n_small, n_big)
    finally:
        e.close()


@pytest.mark.parametrize("cells_level", [None, 2], ids=["production", "cells-config-stops-at-level-2"])
def test_packed_row_filter_is_bit_identical_to_one_pair_per_wave(monkeypatch, stack, cells_level):
    """cells_level 2: the planes that choose the cells config filter levels 1 and 2 only -- levels 3 and 4 are inactive
    for them and the packed kernel writes rows of zeros, for the others it filters."""
    cells_cfg = dict(synth.CELLS_CONFIG, level=cells_level)
    multi = _run(monkeypatch, stack, cells_cfg, {"DSX_NO_ROW_PACK": "1"})
    assert multi[3] == (0, 0)  # never with the switch
    cfg = multi[2]
    assert 0 < cfg.sum() < N  # both config outcomes
    np.testing.assert_array_equal(multi[1][:8], multi[0])  # the same planes, through the other launch shape
    assert not np.array_equal(multi[1][1], np.minimum(stack[1].astype(np.int64) + 2, 65535))  # the filter did filter
    for env, launches in (({}, None), ({"DSX_ROW_PACK_FILL": "0"}, (1, 4)), ({"DSX_ROW_PACK": "4", "DSX_ROW_PACK_FILL": "0"}, (1, 4))):
        got = _run(monkeypatch, stack, cells_cfg, env)
        # the packed kernel ran: once for the small cohort, once per part of the big one
        if launches is not None:
            assert got[3] == launches, (env, got[3])
        np.testing.assert_array_equal(got[2], cfg, err_msg=str(env))
        np.testing.assert_array_equal(got[0], multi[0], err_msg=str(env))
        np.testing.assert_array_equal(got[1], multi[1], err_msg=str(env))
    if cells_level is None:  # and the reference: a plane of each config against the oracle
        for k in (0, 1):
            ref = orc.filter_stripes(stack[k], "t", synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, synth.ZARR_PATH_HIGH_INT)
            d = np.abs(got[1][k].astype(np.int64) - ref.astype(np.uint16).astype(np.int64))
            assert d.max() <= 1, (k, int(d.max()))


def test_default_packs_a_launch_that_fills_the_chip(monkeypatch):
    """16 planes of 2048^2 (4224 row pairs on levels 3 ... 8: 16 waves per CU and more on chips of up to 264 CUs) take the
    packed kernel without any switch, 2 planes do not; same bits as with DSX_NO_ROW_PACK=1."""
    h = w = 2048
    planes = synth.synthetic_bank(4, h, w)
    planes = np.concatenate([planes] * 4)
    res = {}
    for mode in ("0", "1"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("DSX_NO_ROW_PACK", mode)
        e = eng_mod.DestripeEngine(0)
        try:
            e.plan(h, w, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=16)
            two = np.asarray(e.run(planes[:2], out_dtype=np.uint16))
            n_two = e.row_pack_launches()
            full = np.asarray(e.run(planes, out_dtype=np.uint16))
            res[mode] = (two, full, n_two, e.row_pack_launches() - n_two)
        finally:
            e.close()
    assert res["0"][2:] == (0, 1) and res["1"][2:] == (0, 0), (res["0"][2:], res["1"][2:])
    np.testing.assert_array_equal(res["0"][0], res["1"][0])
    np.testing.assert_array_equal(res["0"][1], res["1"][1])
