"""NumPy restatement of the options of the dual-band filter (README "filter_streaks": one-sided bands, a smoothed
blend weight, dark / flat), on ``streaks_oracle.subband``; pinned against the real libraries by
``tests/golden/streaks_options.npz`` (``tools/make_golden_streaks_options.py``)."""

import os

import numpy as np

from aind_smartspim_destripe_amd import wavelets
from oracle import destripe_oracle as orc
from tests import streaks_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaks_options.npz")


def fold(i, n):
    """Half-sample reflection (``d c b a | a b c d | d c b a``) of any index onto ``[0, n)``."""
    i = np.asarray(i) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def smooth(w, s, truncate=4.0):
    """``scipy.ndimage.gaussian_filter(w, s)`` with its defaults: two 1-D passes, radius ``int(4 s + 0.5)``, taps
    ``exp(-k^2 / 2 s^2)`` normalised to sum 1, borders folded (as often as an axis shorter than the radius needs)."""
    r = int(truncate * s + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / s) ** 2)
    k /= k.sum()
    out = np.asarray(w, dtype=np.float64)
    for ax in (0, 1):
        n = out.shape[ax]
        idx = fold(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], n)
        out = np.tensordot(np.take(out, idx, axis=ax), k, axes=([ax + 1], [0]))
    return out


def shade(r, flat, dark):
    """The reference's ``flatfield_correction(r, flat, dark)`` before its cast: the clipped float."""
    r = np.asarray(r, dtype=np.float64)
    d = np.asarray(dark, dtype=np.float64)[: r.shape[0], : r.shape[1]]
    return np.clip(np.where(r > d, r - d, 0.0) / np.asarray(flat, dtype=np.float64), 0, 65535)


def bands(img, sigma, level=0, wavelet="db3", threshold=-1):
    """``(t, x, f, b)``: the threshold, the float64 plane and the filtered bands cropped to ``[H, W]`` (``None`` for a
    band whose sigma is ``None``)."""
    img = np.asarray(img)
    bank = wavelets.filter_bank(wavelet)
    t = threshold if threshold != -1 else so.threshold_otsu(img)[0]
    H, W = img.shape
    x = img.astype(np.float64)
    xp = np.pad(x, ((0, H & 1), (0, W & 1)), mode="edge")
    fg, bg = sigma
    f = None if fg is None else so.subband(np.maximum(xp, t), fg, level, bank)[:H, :W]
    b = None if bg is None else so.subband(np.minimum(xp, t), bg, level, bank)[:H, :W]
    return float(t), x, f, b


def blend(x, f, b, t, crossover=10, smoothing=0, flat=None, dark=None):
    w = orc.foreground_fraction(x, t, crossover)
    if smoothing > 0:
        w = smooth(w, smoothing)
    r = (x if f is None else f) * w + (x if b is None else b) * (1 - w)
    return r if flat is None else shade(r, flat, dark)


def filter_streaks(img, sigma, level=0, wavelet="db3", crossover=10, threshold=-1, smoothing=0, flat=None, dark=None):
    """Returns ``(t, out[H, W] float64)``; ``sigma``: a pair of two different sigmas, one of them may be ``None``."""
    t, x, f, b = bands(img, sigma, level, wavelet, threshold)
    return t, blend(x, f, b, t, crossover, smoothing, flat, dark)


def golden_cases(path=GOLDEN):
    """The golden cases as dicts (``flat`` / ``dark``: ``None`` where the case has no shading)."""
    cases = []
    with np.load(path) as z:
        for name in z["names"]:
            name = str(name)
            cases.append({
                "name": name,
                "image": z[name + "/image"],
                "sigma": tuple(None if np.isnan(v) else float(v) for v in z[name + "/sigma"]),
                "level": int(z[name + "/level"]),
                "wavelet": str(z[name + "/wavelet"]),
                "crossover": float(z[name + "/crossover"]),
                "threshold": float(z[name + "/threshold"]),
                "smoothing": float(z[name + "/smoothing"]),
                "flat": z[name + "/flat"] if name + "/flat" in z.files else None,
                "dark": z[name + "/dark"] if name + "/dark" in z.files else None,
                "t": float(z[name + "/t"]),
                "out": z[name + "/out"],
                "out_u16": z[name + "/out_u16"],
            })  # fmt: skip
    return cases


def case_kwargs(case):
    """Arguments of ``filtering.destripe_streaks_planes`` / ``filter_streaks`` for a golden case."""
    return dict(sigma=case["sigma"], level=case["level"], wavelet=case["wavelet"], crossover=case["crossover"],
                threshold=case["threshold"], smoothing=case["smoothing"], flat=case["flat"], dark=case["dark"])  # fmt: skip
