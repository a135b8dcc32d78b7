"""Write tests/golden/streaks_options.npz: the options of the dual-band filter (one-sided bands, a smoothed blend
weight, dark / flat; README "filter_streaks") run with the real libraries.

Run with the interpreter that has the reference's pinned stack (PyWavelets 1.1.1, SciPy 1.7.1, scikit-image
0.18.3), from the repository root:

    python3.9 tools/make_golden_streaks_options.py /path/to/aind-smartspim-destripe/code

The bands are those of tools/make_golden_streaks.py (``pywt``, ``scipy.fftpack``, the reference's ``gaussian_filter``
notch); the weight is ``scipy.ndimage.gaussian_filter(ref.foreground_fraction(x, t, crossover), smoothing)`` on the
unpadded plane, and the dark / flat step is the reference's ``flatfield_correction``.  pystripe itself is not run.
Every case records its input, its arguments (a sigma that is not filtered: nan), t, the float64 result ``out`` (with
a flat: the clipped value before the reference's cast) and ``out_u16`` (clip + truncate; with a flat the very array
``flatfield_correction`` returned).
"""

import os
import sys

import numpy as np


def main(ref_code):
    sys.path.insert(0, ref_code)
    import pywt
    from scipy import fftpack, ndimage
    from skimage import filters

    from aind_smartspim_destripe import filtering as ref

    def subband(z, sigma, level, wavelet):
        y = np.log(1 + z)
        w = pywt.Wavelet(wavelet)
        if level in (0, None):
            level = pywt.dwt_max_level(min(y.shape), w.dec_len)
        coeffs = pywt.wavedec2(y, w, mode="symmetric", level=level)
        out = [coeffs[0]]
        for ch, cv, cd in coeffs[1:]:
            s = ch.shape[0] * sigma / y.shape[0]
            fch = fftpack.rfft(ch, axis=-1)
            ch = fftpack.irfft(fch * ref.gaussian_filter(ch.shape, s), axis=-1)
            out.append((ch, cv, cd))
        return np.exp(pywt.waverec2(out, w)) - 1

    def streaks(img, sigma, level, wavelet, crossover, threshold, smoothing, flat, dark):
        t = threshold if threshold != -1 else filters.threshold_otsu(img)
        H, W = img.shape
        x0 = img.astype(np.float64)
        x = np.pad(x0, ((0, H & 1), (0, W & 1)), mode="edge")
        fg, bg = sigma
        f = x0 if fg is None else subband(np.maximum(x, t), fg, level, wavelet)[:H, :W]
        b = x0 if bg is None else subband(np.minimum(x, t), bg, level, wavelet)[:H, :W]
        w = ref.foreground_fraction(x0, t, crossover)
        if smoothing > 0:
            w = ndimage.gaussian_filter(w, smoothing)
        r = f * w + b * (1 - w)
        if flat is None:
            return float(t), r, np.clip(r, 0, 65535).astype(np.uint16)
        u16 = ref.flatfield_correction(r.copy(), flat, dark)
        d = dark[:H, :W]
        clipped = np.clip(np.where(r > d, r - d, 0.0) / flat, 0, 65535)
        assert u16.dtype == np.uint16 and np.array_equal(u16, clipped.astype(np.uint16))
        return float(t), clipped, u16

    rng = np.random.default_rng(20261020)

    def plane_u16(h, w):
        base = rng.poisson(180.0, size=(h, w)).astype(np.float64)
        cells = rng.random((h, w)) < 0.03
        base[cells] += rng.poisson(900.0, size=int(cells.sum()))
        base += 40.0 * np.sin(np.arange(h) / 3.0)[:, None]  # horizontal streaks
        return np.clip(base, 0, 65535).astype(np.uint16)

    def plane_f32(h, w):
        base = rng.normal(150.0, 12.0, size=(h, w))
        cells = rng.random((h, w)) < 0.2
        base[cells] = rng.normal(700.0, 60.0, size=int(cells.sum()))
        base += 25.0 * np.sin(np.arange(h) / 2.5)[:, None]
        return np.maximum(base, 0.0).astype(np.float32)

    def shading(h, w, dark_shape):
        # a flat in [0.8, 1.2] and a dark of 100 on a plane larger than the image (cropped by indexing); the shaded
        # values of these planes stay below 9 000
        flat = (0.8 + 0.4 * rng.random((h, w))).astype(np.float32)
        return flat, np.full(dark_shape, 100.0, dtype=np.float32)

    a = plane_u16(64, 96)
    flat_a, dark_a = shading(64, 96, (70, 100))
    b = plane_u16(33, 47)
    flat_b, dark_b = shading(33, 47, (40, 48))
    c = plane_u16(20, 6)
    d = plane_f32(64, 96)
    cases = [
        # (name, image, sigma, level, wavelet, crossover, threshold, smoothing, flat, dark)
        ("u16_64x96_plain", a, (8.0, 16.0), 0, "db3", 10.0, -1, 0.0, None, None),
        ("u16_64x96_smooth1", a, (8.0, 16.0), 0, "db3", 10.0, -1, 1.0, None, None),
        ("u16_64x96_fg", a, (8.0, None), 0, "db3", 10.0, -1, 0.0, None, None),
        ("u16_64x96_bg", a, (None, 16.0), 0, "db3", 10.0, -1, 0.0, None, None),
        ("u16_64x96_fg_smooth1", a, (8.0, None), 0, "db3", 10.0, -1, 1.0, None, None),
        ("u16_64x96_smooth1_shaded", a, (8.0, 16.0), 0, "db3", 10.0, -1, 1.0, flat_a, dark_a),
        ("u16_64x96_shaded", a, (8.0, 16.0), 0, "db3", 10.0, -1, 0.0, flat_a, dark_a),
        ("u16_33x47_sym4_smooth1_shaded", b, (8.0, 16.0), 2, "sym4", 10.0, -1, 1.0, flat_b, dark_b),
        ("u16_20x6_haar_smooth2", c, (8.0, 16.0), 0, "haar", 10.0, -1, 2.0, None, None),
        ("f32_64x96_fg_fixed_t", d, (8.0, None), 0, "db3", 10.0, 300.5, 0.0, None, None),
    ]
    out = {"names": np.array([c[0] for c in cases])}
    for name, img, sigma, level, wavelet, crossover, threshold, smoothing, flat, dark in cases:
        t, res, u16 = streaks(img, sigma, level, wavelet, crossover, threshold, smoothing, flat, dark)
        out[name + "/image"] = img
        out[name + "/sigma"] = np.array([np.nan if s is None else s for s in sigma], dtype=np.float64)
        out[name + "/level"] = np.array(level)
        out[name + "/wavelet"] = np.array(wavelet)
        out[name + "/crossover"] = np.array(crossover, dtype=np.float64)
        out[name + "/threshold"] = np.array(threshold, dtype=np.float64)
        out[name + "/smoothing"] = np.array(smoothing, dtype=np.float64)
        if flat is not None:
            out[name + "/flat"] = flat
            out[name + "/dark"] = dark
        out[name + "/t"] = np.array(t, dtype=np.float64)
        out[name + "/out"] = res
        out[name + "/out_u16"] = u16
        print(name, img.shape, img.dtype, "t =", t, "out range", float(res.min()), float(res.max()))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "streaks_options.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_CODE", "code"))
