"""Two contexts with different launch switches in ONE process and thread: each follows its own switches at every call
(the launch helpers take the context's tuning as an argument; there is no per-thread "current tuning"), and the
switches move no bit of a result."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = {"DSX_ROW_WPB": "4", "DSX_NO_FUSE": "1", "DSX_SEG_MIN_ROWS": "24"}


def test_two_contexts_keep_their_own_switches():
    from aind_smartspim_destripe_amd import engine as eng_mod, synth

    saved = {k: os.environ.get(k) for k in SWITCHES}
    a = b = None
    try:
        os.environ.update(SWITCHES)  # dsx_init reads the switches once, per context
        a = eng_mod.DestripeEngine(0)
        for k in SWITCHES:
            os.environ.pop(k)
        b = eng_mod.DestripeEngine(0)
        planes = synth.synthetic_bank(3, 96, 128)
        for e in (a, b):
            e.plan(96, 128, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT, max_batch=3)
        outs = [e.run(planes, out_dtype=np.uint16) for e in (a, b, a, b)]
        # what is observable of the chain without a trace: launches per kernel class of a profiled run.  B fuses
        # levels 1 and 2 into the level-1 launch, A (DSX_NO_FUSE) runs level 2 as one more coarse launch
        counts = []
        for e in (a, b):
            e.profile(True)
            e.run(planes, out_dtype=np.uint16)
            counts.append({k: v[1] for k, v in e.profile_read().items()})
            e.profile(False)
        b.close()
        b = None
        outs.append(a.run(planes, out_dtype=np.uint16))  # A still follows its switches after B is gone
        for k, out in enumerate(outs[1:]):
            assert np.array_equal(out, outs[0]), "run %d differs from run 0" % (k + 1)
        print("launches per class  A:", counts[0], " B:", counts[1])
        assert counts[0]["k_fwd_march(coarse)"] == counts[1]["k_fwd_march(coarse)"] + 1, counts
        assert counts[0]["k_fwd_march(level1)"] == counts[1]["k_fwd_march(level1)"] == 1, counts
    finally:
        for e in (a, b):
            if e is not None:
                e.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
