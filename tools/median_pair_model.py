#!/usr/bin/env python3
"""What the median loop of rf_pair_body (csrc/dsx_kernels.h) counts per row PAIR: a wave filters two coefficient rows and
runs the bracketing of tools/median_model.py::kernel_median3 for both.  A median is read only at masked positions, so

  now        both rows of a pair with any masked entry are counted until BOTH are finished (DSX_MEDIAN_LOCKSTEP=1);
  need       a row without a masked entry is left out, two masked rows still run in lockstep;
  need+stop  as shipped: a row is counted only while it is needed and not finished.

Unit: row-count-passes (one row counted once, the two zero-spike probes included), over the pairs that enter the loop.
Rows: levels 1 and 2 of 2048 x 2048 planes of the synthetic bank through the oracle's stages, no-cells config.  Every
median of a needed row is checked against np.median.
usage: python tools/median_pair_model.py [plane ...] > profiles/median_rows_model.txt   (CPU only; nothing in the product
imports it)"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from aind_smartspim_destripe_amd import synth
from oracle import destripe_oracle as orc
from median_model import kernel_median3

PLANES = (0, 3, 5, 9, 17, 26)


def pair_kinds(ch, thr):
    """(pairs with no, one, two masked rows) of a level's coefficients, paired as the kernels pair them: rows 2 p and
    2 p + 1, the partner of a last odd row being a row of zeros."""
    masked = (np.abs(ch) > thr).any(axis=1)
    if masked.size & 1:
        masked = np.append(masked, False)
    n = masked[0::2].astype(int) + masked[1::2].astype(int)
    return int((n == 0).sum()), int((n == 1).sum()), int((n == 2).sum())


def level_passes(ch, thr):
    """(now, need, need+stop, bad medians) of one level."""
    ch = ch.astype(np.float32); thr = np.float32(thr)
    mask = np.abs(ch) > thr
    bg = np.where(mask, np.float32(0), ch)
    h = ch.shape[0]
    now = need = stop = bad = 0
    for p in range((h + 1) // 2):
        rows = [bg[2 * p], bg[2 * p + 1] if 2 * p + 1 < h else np.zeros_like(bg[0])]
        m = [bool(mask[2 * p].any()), 2 * p + 1 < h and bool(mask[2 * p + 1].any())]
        if not (m[0] or m[1]):
            continue
        n = []
        for r in range(2):
            med, cnt = kernel_median3(rows[r], thr)
            n.append(cnt)
            if m[r] and med != np.float32(np.median(rows[r])):
                bad += 1
        now += 2 * max(n)
        need += 2 * max(n) if (m[0] and m[1]) else n[0 if m[0] else 1]
        stop += sum(n[r] for r in range(2) if m[r])
    return now, need, stop, bad


if __name__ == "__main__":  # pragma: no cover
    planes = [int(a) for a in sys.argv[1:]] or PLANES
    print("plane level rows_masked pairs0 pairs1 pairs2 now need need+stop need/now need+stop/now bad_medians")
    for k in planes:
        plane = synth.synthetic_plane(k, 2048, 2048)
        _, stages = orc.log_space_fft_filtering(plane, return_stages=True, **synth.NO_CELLS_CONFIG)
        stages = stages[::-1]  # fine -> coarse
        for lv in (0, 1):
            ch, thr = stages[lv]["ch"], stages[lv]["threshold"]
            frac = float((np.abs(ch) > thr).any(axis=1).mean())
            k0, k1, k2 = pair_kinds(ch, thr)
            now, need, stop, bad = level_passes(ch, thr)
            print("{:5d} {:5d} {:11.2f} {:6d} {:6d} {:6d} {:5d} {:5d} {:9d} {:8.2f} {:13.2f} {:11d}".format(
                k, lv + 1, frac, k0, k1, k2, now, need, stop, need / max(now, 1), stop / max(now, 1), bad), flush=True)
