"""Planes and the float64 model of the march route of the dual-band filter (``route="march"``), shared by
tests/test_streaks_march_model.py and the GPU tests of the route."""

import numpy as np

from oracle import destripe_oracle as orc
from tests import streaks_oracle as so


def plane(seed, h, w, dtype=np.uint16):
    """Poisson(150) x a gain per row exp(0.15 N), one 10 x 10 square of +4000."""
    rng = np.random.default_rng(seed)
    img = rng.poisson(150.0, size=(h, w)).astype(np.float64) * np.exp(0.15 * rng.standard_normal(h))[:, None]
    y, x = int(rng.integers(0, h - 10)), int(rng.integers(0, w - 10))
    img[y : y + 10, x : x + 10] += 4000.0
    img = np.clip(np.floor(img), 0, 65535)
    return img.astype(dtype)


def level_shapes(shape, level, filter_len=6):
    """cH shapes of ``wavedec2(level)``, coarse to fine (the order of the oracle's ``mask_overrides``)."""
    n = level if level else so.max_level(shape, filter_len)
    h, w = shape
    out = []
    for _ in range(n):
        h, w = orc.dwt_coeff_len(h, filter_len), orc.dwt_coeff_len(w, filter_len)
        out.append((h, w))
    return out[::-1]


def band(z, sigma, level=0):
    """One band as the march route computes it: the log-space filter with sigma rescaled to its normalisation of ``s``
    and every level's mask forced empty, minus 2."""
    H, W = z.shape
    masks = [np.zeros(s, dtype=bool) for s in level_shapes(z.shape, level)]
    out = orc.log_space_fft_filtering(z, wavelet="db3", level=level if level else None, sigma=sigma * min(H, W) / H,
                                      mask_overrides=masks)  # fmt: skip
    return out - 2.0


def march_model(img, sigma, level=0, crossover=10, threshold=-1):
    """``(t, out)`` of the filter written as the march route runs it (even planes, db3), float64."""
    img = np.asarray(img)
    assert img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0
    t = threshold if threshold != -1 else so.threshold_otsu(img)[0]
    x = img.astype(np.float64)
    fg, bg = sigma
    if fg == bg:
        return float(t), band(x, fg, level)
    w = orc.foreground_fraction(x, t, crossover)
    return float(t), band(np.maximum(x, t), fg, level) * w + band(np.minimum(x, t), bg, level) * (1 - w)
