"""CPU, float64: the identity the march route of the dual-band filter rests on.  For an even plane, db3 and an empty
mask, ``log_space_fft_filtering(z, level, sigma * min(H, W) / H) - 2`` is the band of ``filter_streaks`` -- the row
filters are the same packed-index notch, only the normalisation of ``s`` differs, the median in-paint vanishes with the
mask, and ``exp(y) + 1`` against ``exp(y) - 1`` is the 2.  Bound: 1e-12 (1 + |ref|) on every pixel."""

import numpy as np
import pytest

from tests import streaks_march_cases as mc
from tests import streaks_oracle as so

SHAPES = [((64, 64), np.uint16), ((96, 128), np.uint16), ((64, 2048), np.uint16), ((130, 250), np.uint16),
          ((402, 2000), np.uint16), ((128, 96), np.float32)]  # fmt: skip


def _check(img, sigma, **kw):
    t_ref, ref = so.filter_streaks(img, sigma, **kw)
    t, out = mc.march_model(img, sigma, **kw)
    assert t == t_ref
    err = np.abs(out - ref) / (1.0 + np.abs(ref))
    assert err.max() <= 1e-12, float(err.max())


@pytest.mark.parametrize("shape,dtype", SHAPES, ids=["{}x{}-{}".format(s[0], s[1], np.dtype(d).name) for s, d in SHAPES])
def test_bands_of_the_log_space_filter_are_the_dual_band_filter(shape, dtype):
    img = mc.plane(shape[0] + shape[1], shape[0], shape[1], dtype)
    if dtype == np.float32:
        img = img + np.float32(0.25)  # off the integers: t is a bin centre of the 256-bin histogram
        assert so.threshold_otsu(img)[0] != np.floor(so.threshold_otsu(img)[0])
    _check(img, (8.0, 16.0))


def test_single_band_level_and_fixed_threshold():
    img = mc.plane(5, 96, 128)
    _check(img, (12.0, 12.0))
    _check(img, (8.0, 16.0), level=2)
    _check(img, (8.0, 16.0), threshold=300)
    _check(img, (8.0, 16.0), threshold=300.5, level=2, crossover=4)
