"""Write tests/golden/lightsheet.npz: the cases of tests/lightsheet_cases.py run through the library the light-sheet
background mode is built on, scikit-image's ``rank.percentile``.

Run with the interpreter that has the reference's pinned stack (scikit-image 0.18.3), from the repository root:

    python3.9 tools/make_golden_lightsheet.py

Per case ``<name>``: ``<name>_x`` the uint16 plane, ``<name>_args`` = (p, A, B, lambda) as float64, ``<name>_q`` the
quantised plane (step 1 in NumPy float64), ``<name>_ls`` = ``rank.percentile(q, ones((1, A)), p0=p)`` and ``<name>_bg``
= ``rank.percentile(q, ones((B, B)), p0=p)`` from the real library, and ``<name>_out``: step 3 (the NumPy restatement
``lightsheet_cases.subtract_numpy``) over those two planes.  ``skimage_version`` records the library.  pystripe itself
is not run.  The tool also counts the pixels at which the restatement of step 2 (``percentile_numpy``) differs from the
library and refuses to write a fixture its own restatement does not reproduce.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import skimage
    from skimage.filters import rank

    import lightsheet_cases as lc

    out = {"skimage_version": np.array(skimage.__version__), "names": np.array(lc.case_names())}
    differing = 0
    for name, x, prm in lc.cases():
        p, A, B = prm["percentile"], prm["artifact_length"], prm["background_window_size"]
        lam = prm["lightsheet_vs_background"]
        q = lc.quantise(x)
        ls = rank.percentile(q, np.ones((1, A), np.uint8), p0=p)
        bg = rank.percentile(q, np.ones((B, B), np.uint8), p0=p)
        assert ls.dtype == np.uint8 and bg.dtype == np.uint8
        d = int((lc.percentile_numpy(q, 1, A, p) != ls).sum()) + int((lc.percentile_numpy(q, B, B, p) != bg).sum())
        print("{:8s} {:4d} x {:4d}  A {:4d}  B {:3d}  p {:.2f}: {} pixels differ from the restatement".format(
            name, x.shape[0], x.shape[1], A, B, p, d))  # fmt: skip
        differing += d
        out[name + "_x"] = x
        out[name + "_args"] = np.array([p, A, B, lam], np.float64)
        out[name + "_q"] = q
        out[name + "_ls"] = ls
        out[name + "_bg"] = bg
        out[name + "_out"] = lc.subtract_numpy(x, ls, bg, lam)
    if differing:
        raise SystemExit("the restatement differs from scikit-image at {} pixels: correct it first".format(differing))
    path = os.path.join(REPO, "tests", "golden", "lightsheet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; scikit-image", skimage.__version__)


if __name__ == "__main__":
    main()
