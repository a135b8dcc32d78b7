"""Write tests/golden/streaks.npz and streaks_256.npz: the dual-band wavelet-FFT filter (filter_streaks with sigma = (fg, bg)) run with
the real libraries.

Run with the interpreter that has the reference's pinned stack (PyWavelets 1.1.1, SciPy 1.7.1, scikit-image
0.18.3), from the repository root:

    python3.9 tools/make_golden_streaks.py /path/to/aind-smartspim-destripe/code

Steps 1-5 of README "filter_streaks" are composed from the reference's own ``notch`` / ``gaussian_filter`` /
``foreground_fraction`` (imported from its ``aind_smartspim_destripe.filtering``), ``pywt``, ``scipy.fftpack`` and
``skimage.filters.threshold_otsu``.  Every case records its input, t, the Otsu bin (float32 inputs: the index into
the 256 bin centres; uint16: t - min) and the float64 output.
"""

import os
import sys

import numpy as np


def main(ref_code):
    sys.path.insert(0, ref_code)
    import pywt
    from scipy import fftpack
    from skimage import filters
    from skimage.exposure import histogram

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

    def streaks(img, sigma, level, wavelet, crossover, threshold):
        t = threshold if threshold != -1 else filters.threshold_otsu(img)
        H, W = img.shape
        x = np.pad(img.astype(np.float64), ((0, H & 1), (0, W & 1)), mode="edge")
        fg, bg = sigma
        if fg == bg:
            out = subband(x, fg, level, wavelet)
        else:
            b = subband(np.minimum(x, t), bg, level, wavelet)
            f = subband(np.maximum(x, t), fg, level, wavelet)
            w = ref.foreground_fraction(x, t, crossover)
            out = f * w + b * (1 - w)
        return float(t), out[:H, :W]

    def otsu_bin(img, t):
        if np.all(img == img.ravel()[0]):
            return 0
        if img.dtype == np.uint16:
            return int(t) - int(img.min())
        _, centres = histogram(img.ravel(), 256, source_range="image")
        return int(np.argmin(np.abs(centres - t)))

    rng = np.random.default_rng(20261016)

    def plane_u16(h, w):
        base = rng.poisson(180.0, size=(h, w)).astype(np.float64)
        cells = rng.random((h, w)) < 0.03
        base[cells] += rng.poisson(900.0, size=int(cells.sum()))
        base += 40.0 * np.sin(np.arange(h) / 3.0)[:, None]  # horizontal streaks
        return np.clip(base, 0, 65535).astype(np.uint16)

    def plane_f32(h, w):
        # two well separated populations: the Otsu curve has one clear maximum (no plateau)
        base = rng.normal(150.0, 12.0, size=(h, w))
        cells = rng.random((h, w)) < 0.2
        base[cells] = rng.normal(700.0, 60.0, size=int(cells.sum()))
        base += 25.0 * np.sin(np.arange(h) / 2.5)[:, None]
        return np.maximum(base, 0.0).astype(np.float32)

    cases = []
    # (name, image, sigma, level, wavelet, crossover, threshold)
    cases.append(("db3_64_u16", plane_u16(64, 64), (8.0, 16.0), 0, "db3", 10.0, -1))
    cases.append(("db3_96x130_f32", plane_f32(96, 130), (12.0, 24.0), 0, "db3", 10.0, -1))
    cases.append(("db3_127x201_u16_odd", plane_u16(127, 201), (16.0, 32.0), 0, "db3", 25.0, -1))
    cases.append(("db3_63x101_f32_odd", plane_f32(63, 101), (16.0, 32.0), 3, "db3", 10.0, -1))
    cases.append(("db3_256_u16", plane_u16(256, 256), (32.0, 64.0), 0, "db3", 10.0, -1))
    cases.append(("db3_80_f32_level2", plane_f32(80, 80), (32.0, 64.0), 2, "db3", 50.0, -1))
    cases.append(("haar_48x66_u16", plane_u16(48, 66), (12.0, 24.0), 0, "haar", 10.0, -1))
    cases.append(("sym4_48x66_f32", plane_f32(48, 66), (12.0, 24.0), 3, "sym4", 10.0, -1))
    cases.append(("db3_64_u16_single", plane_u16(64, 64), (10.0, 10.0), 0, "db3", 10.0, -1))
    cases.append(("db3_48x66_f32_single", plane_f32(48, 66), (20.0, 20.0), 2, "db3", 10.0, -1))
    cases.append(("db3_48x66_u16_fixed_t", plane_u16(48, 66), (12.0, 24.0), 0, "db3", 10.0, 300.0))
    cases.append(("db3_64_u16_constant", np.full((64, 64), 321, np.uint16), (8.0, 16.0), 0, "db3", 10.0, -1))
    cases.append(("db3_64x95_u16_odd_width", plane_u16(64, 95), (8.0, 16.0), 0, "db3", 10.0, -1))
    cases.append(("db3_75x64_f32_odd_height", plane_f32(75, 64), (8.0, 16.0), 0, "db3", 25.0, -1))

    # no committed file may exceed 1 MiB: the 256 x 256 cases go to a second file
    files = {"streaks.npz": [c for c in cases if c[1].shape != (256, 256)],
             "streaks_256.npz": [c for c in cases if c[1].shape == (256, 256)]}  # fmt: skip
    for fname, group in files.items():
        out = {"names": np.array([c[0] for c in group])}
        for name, img, sigma, level, wavelet, crossover, threshold in group:
            t, res = streaks(img, sigma, level, wavelet, crossover, threshold)
            out[name + "/image"] = img
            out[name + "/sigma"] = np.array(sigma, dtype=np.float64)
            out[name + "/level"] = np.array(level)
            out[name + "/wavelet"] = np.array(wavelet)
            out[name + "/crossover"] = np.array(crossover, dtype=np.float64)
            out[name + "/threshold"] = np.array(threshold, dtype=np.float64)
            out[name + "/t"] = np.array(t, dtype=np.float64)
            out[name + "/otsu_bin"] = np.array(otsu_bin(img, t) if threshold == -1 else -1)
            out[name + "/out"] = res
            print(name, img.shape, img.dtype, "t =", t, "out range", float(res.min()), float(res.max()))
        dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", fname)
        np.savez_compressed(dst, **out)
        print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_CODE", "code"))
