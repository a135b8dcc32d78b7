#!/usr/bin/env python
"""Writes tests/golden/flat_estimation.npz: scipy.ndimage.gaussian_filter (defaults) of five small float64 planes, what
``flatfield_estimation.gaussian_smooth`` restates in NumPy (tests/test_flatfield_estimation.py).  Needs SciPy; the
product does not.  The SciPy version is recorded in the file.

    python tools/make_golden_flat_estimation.py
"""

import os

import numpy as np
import scipy
from scipy import ndimage

CASES = [((24, 40), 1.5), ((24, 40), 32.0), ((7, 9), 3.0), ((1, 5), 2.0), ((33, 1), 4.0)]
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "flat_estimation.npz")


def main():
    rs = np.random.RandomState(2024)
    arrays = {"scipy_version": np.array(scipy.__version__), "n_cases": np.array(len(CASES))}
    for i, (shape, sigma) in enumerate(CASES):
        plane = np.floor(rs.rand(*shape) * 4000.0)  # whole counts, as a rank plane holds them
        arrays["plane_{}".format(i)] = plane
        arrays["sigma_{}".format(i)] = np.array(sigma)
        arrays["smooth_{}".format(i)] = ndimage.gaussian_filter(plane, sigma)
    np.savez(OUT, **arrays)
    print("wrote", OUT, "with SciPy", scipy.__version__)


if __name__ == "__main__":
    main()
