"""GPU: the dual-band wavelet-FFT filter (``filter_streaks`` with ``sigma = (fg, bg)``) against the real-library
fixtures and the NumPy restatement.  Bound everywhere: |gpu - ref| <= 1e-4 (1 + |ref|) for every pixel."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import filtering
from tests import streaks_oracle as so

pytestmark = pytest.mark.gpu

GOLDEN = [os.path.join(os.path.dirname(__file__), "golden", f) for f in ("streaks.npz", "streaks_256.npz")]
CASES = list(so.golden_cases(GOLDEN))


def _within(gpu, ref):
    err = np.abs(gpu.astype(np.float64) - ref) / (1.0 + np.abs(ref))
    assert err.max() <= 1e-4, float(err.max())


def _args(c):
    return dict(level=c["level"], wavelet=c["wavelet"], crossover=c["crossover"], threshold=c["threshold"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case(case):
    out = filtering.filter_streaks(case["image"], sigma=case["sigma"], **_args(case))
    assert out.dtype == np.float64 and out.shape == case["image"].shape
    _within(out, case["out"])
    _, t = filtering.destripe_streaks_planes(case["image"][None], case["sigma"], out_dtype=np.float32,
                                             return_threshold=True, **_args(case))  # fmt: skip
    if case["image"].dtype == np.uint16 or case["threshold"] != -1:
        assert t[0] == case["t"]
    else:  # float32: the same bin centre (float32 edges)
        assert np.float32(t[0]) == np.float32(case["t"])


def _plane(rng, h, w, dtype):
    base = rng.poisson(200.0, size=(h, w)).astype(np.float64)
    cells = rng.random((h, w)) < 0.05
    base[cells] += rng.poisson(1500.0, size=int(cells.sum()))
    base += 50.0 * np.sin(np.arange(h) / 4.0)[:, None]
    base = np.clip(base, 0, 65535)
    return base.astype(np.uint16) if dtype == np.uint16 else base.astype(np.float32)


@pytest.mark.parametrize("shape,dtype", [((2048, 2048), np.uint16), ((1600, 2000), np.float32)])
def test_large_planes_against_restatement(shape, dtype):
    img = _plane(np.random.default_rng(7), shape[0], shape[1], dtype)
    sigma = (64.0, 128.0)
    out, t = filtering.destripe_streaks_planes(img[None], sigma, out_dtype=np.float32, return_threshold=True)
    t_ref, ref = so.filter_streaks(img, sigma)
    assert np.float32(t[0]) == np.float32(t_ref)
    _within(out[0], ref)


def test_batched_equals_single_plane_calls():
    rng = np.random.default_rng(11)
    planes = np.stack([_plane(rng, 96, 130, np.uint16) for _ in range(40)])
    planes[5] = 400  # a constant plane among them
    sigma = (12.0, 24.0)
    batched, tb = filtering.destripe_streaks_planes(planes, sigma, out_dtype=np.float32, max_batch=32,
                                                    return_threshold=True)  # fmt: skip
    for k in range(40):
        single, ts = filtering.destripe_streaks_planes(planes[k : k + 1], sigma, out_dtype=np.float32, max_batch=1,
                                                       return_threshold=True)  # fmt: skip
        assert np.array_equal(single[0], batched[k]), k
        assert ts[0] == tb[k]
    assert tb[5] == 400.0


def test_uint16_output_is_clip_and_truncate():
    rng = np.random.default_rng(3)
    planes = np.stack([_plane(rng, 127, 201, np.float32) for _ in range(3)])
    planes[1] *= 60.0  # values beyond 65535 after the filter
    f = filtering.destripe_streaks_planes(planes, (16.0, 32.0), out_dtype=np.float32)
    u = filtering.destripe_streaks_planes(planes, (16.0, 32.0), out_dtype=np.uint16)
    assert u.dtype == np.uint16
    assert np.array_equal(u, np.clip(f, 0, 65535).astype(np.uint16))
    assert (u == 65535).any()


def test_single_band_is_subband_of_the_unclipped_plane():
    img = _plane(np.random.default_rng(5), 200, 255, np.uint16)
    out = filtering.filter_streaks(img, sigma=(20.0, 20.0), wavelet="sym4", level=3)
    x = np.pad(img.astype(np.float64), ((0, 0), (0, 1)), mode="edge")
    ref = so.subband(x, 20.0, 3, so.wavelets.filter_bank("sym4"))[:, :255]
    _within(out, ref)


def test_scalar_sigma_is_log_space_filter():
    img = _plane(np.random.default_rng(9), 128, 160, np.uint16)
    a = filtering.filter_streaks(img, sigma=32, level=0, wavelet="db3")
    b = filtering.log_space_fft_filtering(img, sigma=32, level=0, wavelet="db3")
    assert np.array_equal(a, b)


def test_wide_uint16_range_uses_several_histogram_windows():
    # values up to 60 000: ~7 windows of the LDS histogram; t and pixels against the integer Otsu of the restatement
    rng = np.random.default_rng(21)
    img = rng.poisson(300.0, size=(300, 412)).astype(np.float64)
    cells = rng.random(img.shape) < 0.08
    img[cells] = rng.uniform(2000.0, 60000.0, size=int(cells.sum()))
    img = img.astype(np.uint16)
    assert int(img.max()) - int(img.min()) + 1 > 6 * 8192
    out, t = filtering.destripe_streaks_planes(img[None], (16.0, 32.0), out_dtype=np.float32, return_threshold=True)
    t_ref, ref = so.filter_streaks(img, (16.0, 32.0))
    assert t[0] == t_ref and t_ref > 8192  # the maximum lies beyond the first window
    _within(out[0], ref)


def test_one_odd_axis_dual_band_crop():
    for shape in ((64, 95), (75, 64)):
        img = _plane(np.random.default_rng(shape[1]), shape[0], shape[1], np.uint16)
        out = filtering.filter_streaks(img, sigma=(8.0, 16.0))
        _, ref = so.filter_streaks(img, (8.0, 16.0))
        assert out.shape == shape
        _within(out, ref)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -1.0, -3.0])
def test_float32_pixel_without_finite_log_raises(bad):
    img = _plane(np.random.default_rng(1), 64, 64, np.float32)
    img[10, 20] = bad
    with pytest.raises(ValueError, match="not finite"):
        filtering.filter_streaks(img, sigma=(8.0, 16.0), threshold=300.0)
    ok = _plane(np.random.default_rng(2), 64, 64, np.float32)  # the flag does not leak into the next call
    filtering.filter_streaks(ok, sigma=(8.0, 16.0), threshold=300.0)


def test_zero_dimensional_sigma_is_the_scalar_form():
    img = _plane(np.random.default_rng(9), 128, 160, np.uint16)
    a = filtering.filter_streaks(img, sigma=np.array(32.0))
    b = filtering.log_space_fft_filtering(img, sigma=32)
    assert np.array_equal(a, b)
