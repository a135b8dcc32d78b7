"""rf_pair_body (csrc/dsx_kernels.h) runs the exact row median only for the rows that need it: a row of a pair without a
masked entry is never counted, and a row whose bracket is down to one value stops while its partner goes on.  An order
statistic does not depend on which values were probed, so the results must equal, bit for bit,
those of the lockstep loop that counts both rows of a masked pair until both are finished (DSX_MEDIAN_LOCKSTEP=1).

Shapes: 64 x 2048 and 28 x 2048 take k_rowfinal (17 and 8 level-1 row pairs, the last block partial; 28 rows is the height
tests/test_gpu_march_steady_loops.py found sensitive), 200 x 520 the small classes of k_rowfilter with odd coefficient row
counts on some levels (a last pair without a second row), 130 x 516 the merged coarse launch.  Planes: crops of planes 0
(lightly masked: nearly every masked pair has one masked row) and 5 (heavily masked) of the synthetic bank.  Each plane
runs under both production configs (an engine planned with the same config in both slots), alone and in a batch of five.

The CPU part counts, through the oracle's stages, the row pairs with no, one and two masked rows on every level of every
test plane: all three kinds must occur in each shape, or the identity would prove nothing about them.
"""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import synth
from oracle import destripe_oracle as orc
from parity_util import check_plane, gpu_deltas

pytestmark = pytest.mark.gpu

SHAPES = ((64, 2048), (28, 2048), (200, 520), (130, 516))
CONFIGS = {"no_cells": synth.NO_CELLS_CONFIG, "cells": synth.CELLS_CONFIG}
CROPS = ((0, 0), (5, 0), (0, 700), (5, 700), (5, 1400))  # (bank plane, first row of the crop); the first two also run alone
MAX_FLIPS = lambda size: max(3, int(2e-5 * size))  # noqa: E731  (tests/test_gpu_parity.py)

_BANK = {}


def _planes(h, w):
    for k in (0, 5):
        if k not in _BANK:
            _BANK[k] = synth.synthetic_plane(k, 2048, 2048)
    return np.stack([_BANK[k][y0 : y0 + h, :w] for k, y0 in CROPS])


def _pair_kinds(stages):
    """Row pairs with (no, one, two) masked rows over the levels of one plane, paired as the kernels pair them: rows
    2 p and 2 p + 1 of a level, the partner of a last odd row being a row of zeros."""
    kinds = np.zeros(3, dtype=np.int64)
    odd_tail = 0
    for st in stages:
        masked = (np.abs(st["ch"]) > st["threshold"]).any(axis=1)
        if masked.size & 1:
            odd_tail += int(masked[-1])
            masked = np.append(masked, False)
        kinds += np.bincount(masked[0::2].astype(int) + masked[1::2].astype(int), minlength=3)
    return kinds, odd_tail


def _run(h, w, cfg, planes, lockstep, monkeypatch):
    """(each of the first two planes alone, the batch of five) from a fresh engine; the switch is read when it is made"""
    if lockstep:
        monkeypatch.setenv("DSX_MEDIAN_LOCKSTEP", "1")
    else:
        monkeypatch.delenv("DSX_MEDIAN_LOCKSTEP", raising=False)
    e = eng_mod.DestripeEngine(0)
    try:
        e.plan(h, w, cfg, cfg, synth.ZARR_PATH_HIGH_INT, max_batch=len(planes))
        alone = [np.asarray(e.run(planes[k : k + 1], out_dtype=np.uint16)).copy() for k in range(2)]
        batch = np.asarray(e.run(planes, out_dtype=np.uint16)).copy()
    finally:
        e.close()
    return alone, batch


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_needed_rows_only_is_bit_identical_to_the_lockstep_loop(shape, monkeypatch):
    h, w = shape
    planes = _planes(h, w)
    # CPU part: the three kinds of pair occur in this shape's planes
    kinds = np.zeros(3, dtype=np.int64)
    odd_tail = 0
    for name, cfg in CONFIGS.items():
        for k in range(len(planes)):
            _, stages = orc.log_space_fft_filtering(planes[k], return_stages=True, **cfg)
            kk, ot = _pair_kinds(stages)
            kinds += kk
            odd_tail += ot
    print("[median rows] {}x{}: pairs with no / one / two masked rows {}, masked last rows without a partner {}".format(
        h, w, kinds.tolist(), odd_tail))
    assert kinds.min() > 0, (shape, "a kind of row pair does not occur", kinds.tolist())
    if shape == (200, 520):
        assert odd_tail > 0, (shape, "no masked last row without a partner")
    for name, cfg in CONFIGS.items():
        ref_alone, ref_batch = _run(h, w, cfg, planes, True, monkeypatch)
        got_alone, got_batch = _run(h, w, cfg, planes, False, monkeypatch)
        for k in range(2):
            assert np.array_equal(got_alone[k], ref_alone[k]), (shape, name, "plane alone", k)
        assert np.array_equal(got_batch, ref_batch), (shape, name, "batch of five")


def test_parity_of_a_64_by_2048_plane(monkeypatch):
    """The parity statement of tests/parity_util.py with the default setting."""
    monkeypatch.delenv("DSX_MEDIAN_LOCKSTEP", raising=False)
    h, w = 64, 2048
    plane = _planes(h, w)[1]
    e = eng_mod.DestripeEngine(0)
    try:
        deltas = gpu_deltas(e, plane[None])
        out, cfg = e.run(plane[None], out_dtype=np.float32, return_cfg=True)
    finally:
        e.close()
    which, _, _ = orc.select_config(plane, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT)
    assert int(cfg[0]) == which
    check_plane(out[0], plane, deltas[0], "64x2048 plane 5", synth.CELLS_CONFIG if which else synth.NO_CELLS_CONFIG, MAX_FLIPS)
