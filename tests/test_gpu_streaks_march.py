"""GPU: the march route of the dual-band filter (``route="march"``: the bands run through the marching db3 kernels and
the FFT row filter of the log-space engine) against the NumPy restatement called with the engine's own ``t``.
Bound: |gpu - ref| <= 1e-4 (1 + |ref|) on every pixel; ``t`` of both routes is equal bit for bit."""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import filtering, synth
from tests import streaks_march_cases as mc
from tests import streaks_oracle as so

pytestmark = pytest.mark.gpu

SIGMA = (8.0, 16.0)


def _within(gpu, ref):
    err = np.abs(gpu.astype(np.float64) - ref) / (1.0 + np.abs(ref))
    print("max relative error", float(err.max()))
    assert err.max() <= 1e-4, float(err.max())


def _run(img, sigma=SIGMA, route="march", out_dtype=np.float32, **kw):
    out, t = filtering.destripe_streaks_planes(img[None], sigma, out_dtype=out_dtype, return_threshold=True, route=route,
                                               **kw)  # fmt: skip
    return out[0], t[0]


def _against_oracle(img, sigma=SIGMA, **kw):
    out, t = _run(img, sigma, **kw)
    _, t_generic = _run(img, sigma, route="generic", **kw)
    assert np.float32(t) == np.float32(t_generic)  # (both are float32 on the device)
    _, ref = so.filter_streaks(img, sigma, threshold=t, **{k: v for k, v in kw.items() if k != "threshold"})
    assert out.shape == img.shape
    _within(out, ref)
    return out


# 64 x 64; 96 x 128 both element types; W % 4 != 0 (unfused levels, no pair I/O); the 1026-point plan; the embedded,
# swizzled 2048-point plan; a level-1 row wider than one wave (k_rowfilter_wide)
PLANES = [((64, 64), np.uint16), ((96, 128), np.uint16), ((96, 128), np.float32), ((130, 250), np.uint16),
          ((64, 2048), np.uint16), ((66, 2000), np.uint16), ((64, 4800), np.uint16)]  # fmt: skip


@pytest.mark.parametrize("shape,dtype", PLANES, ids=["{}x{}-{}".format(s[0], s[1], np.dtype(d).name) for s, d in PLANES])
def test_march_against_the_restatement(shape, dtype):
    img = mc.plane(shape[0] + shape[1], shape[0], shape[1], dtype)
    if dtype == np.float32:
        img = img + np.float32(0.25)
    _against_oracle(img)


@pytest.mark.parametrize("kw", [dict(level=2), dict(sigma=(12.0, 12.0)), dict(threshold=300), dict(threshold=300.5)],
                         ids=["level2", "equal-sigmas", "t300", "t300.5"])  # fmt: skip
def test_march_variants(kw):
    _against_oracle(mc.plane(7, 96, 128), **kw)


def test_uint16_output_is_clip_and_truncate():
    planes = np.stack([mc.plane(k, 96, 128, np.float32) for k in range(3)])
    planes[1] *= 60.0  # values beyond 65535 after the filter
    f = filtering.destripe_streaks_planes(planes, SIGMA, out_dtype=np.float32, route="march")
    u = filtering.destripe_streaks_planes(planes, SIGMA, out_dtype=np.uint16, route="march")
    assert u.dtype == np.uint16 and (u == 65535).any()
    assert np.array_equal(u, np.clip(f, 0, 65535).astype(np.uint16))
    p16 = np.stack([mc.plane(k, 96, 128) for k in range(3)])
    f = filtering.destripe_streaks_planes(p16, SIGMA, out_dtype=np.float32, route="march")
    u = filtering.destripe_streaks_planes(p16, SIGMA, out_dtype=np.uint16, route="march")
    assert np.array_equal(u, np.clip(f, 0, 65535).astype(np.uint16))


def _batched_equals_single(n, shape, max_batch):
    planes = np.stack([mc.plane(100 + k, shape[0], shape[1]) for k in range(n)])
    batched, tb = filtering.destripe_streaks_planes(planes, SIGMA, out_dtype=np.float32, max_batch=max_batch,
                                                    return_threshold=True, route="march")  # fmt: skip
    assert len(set(tb)) > 1
    for k in range(n):
        single, ts = filtering.destripe_streaks_planes(planes[k : k + 1], SIGMA, out_dtype=np.float32, max_batch=1,
                                                       return_threshold=True, route="march")  # fmt: skip
        assert np.array_equal(single[0], batched[k]), k
        assert ts[0] == tb[k]


@pytest.mark.parametrize("streams", [None, "1"])
def test_five_planes_in_cohorts_of_two_equal_single_plane_calls(monkeypatch, streams):
    filtering.release_engines()  # a context reads DSX_STREAMS when it is created
    if streams:
        monkeypatch.setenv("DSX_STREAMS", streams)
    try:
        _batched_equals_single(5, (96, 128), 2)
    finally:
        filtering.release_engines()


def test_one_call_of_five_planes_on_a_plan_of_two_runs_three_cohorts():
    """The cohort loop inside the library (``n > max_batch`` in one ``dsx_run_host`` / ``dsx_run_device`` call): the
    band planes and the chain's output are reused from cohort to cohort."""
    planes = np.stack([mc.plane(200 + k, 96, 128) for k in range(5)])
    want = filtering.destripe_streaks_planes(planes, SIGMA, out_dtype=np.float32, max_batch=1, route="march")
    e = eng_mod.DestripeEngine(0)
    try:
        e.plan_streaks(96, 128, SIGMA[0], SIGMA[1], max_batch=2, route="march")
        assert e.streaks_route == "march"
        assert np.array_equal(e.run(planes, out_dtype=np.float32), want)
        d_in, d_out = e.alloc(planes.nbytes), e.alloc(want.nbytes)
        try:
            d_in.upload(planes)
            e.run_device(d_in, np.uint16, 5, d_out, np.float32)
            e.sync()
            assert np.array_equal(d_out.download(want.shape, np.float32), want)
        finally:
            d_in.free()
            d_out.free()
        e.plan(96, 128, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, 2700, max_batch=2)
        assert e.streaks_route is None
    finally:
        e.close()


def test_a_cohort_split_over_the_streams_equals_single_plane_calls():
    # 33 planes = 66 virtual planes: four parts of 17, so parts 1 and 3 start at an odd virtual plane
    _batched_equals_single(33, (64, 64), 33)


def test_where_march_does_not_apply():
    img = mc.plane(3, 64, 96)
    with pytest.raises(ValueError, match="march"):
        filtering.filter_streaks(img, sigma=SIGMA, wavelet="haar", route="march")
    odd = np.ascontiguousarray(img[:, :95])
    with pytest.raises(ValueError, match="march"):
        filtering.filter_streaks(odd, sigma=SIGMA, route="march")
    e = eng_mod.DestripeEngine(0)
    try:  # the library refuses what the Python layer refuses
        cfg = eng_mod._StreaksCfg(eng_mod.DSX_WAVELET_DB3, 0, 8.0, 16.0, 10.0, 1, 0.0)
        import ctypes

        assert e._lib.dsx_plan_streaks_ex(e._ctx, 64, 95, 1, ctypes.byref(cfg), 1) == -1
        assert b"even" in e._lib.dsx_last_error(e._ctx)
        assert e._lib.dsx_plan_streaks_ex(e._ctx, 64, 96, 1, ctypes.byref(cfg), 2) == -1
        deep = eng_mod._StreaksCfg(eng_mod.DSX_WAVELET_DB3, 5, 8.0, 16.0, 10.0, 1, 0.0)
        assert e._lib.dsx_plan_streaks_ex(e._ctx, 64, 96, 1, ctypes.byref(deep), 1) == -1
        assert b"level" in e._lib.dsx_last_error(e._ctx)
        assert e.streaks_route is None
    finally:
        e.close()
    for im, kw in ((odd, {}), (img, dict(wavelet="haar"))):
        a = filtering.filter_streaks(im, sigma=SIGMA, route="auto", **kw)
        b = filtering.filter_streaks(im, sigma=SIGMA, route="generic", **kw)
        assert np.array_equal(a, b)
    a = filtering.filter_streaks(img, sigma=SIGMA, route="auto")  # where march applies: the measured choice
    b = filtering.filter_streaks(img, sigma=SIGMA, route=eng_mod.AUTO_ROUTE)
    assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="march"):  # a level beyond the maximum (3 for 64 x 96)
        filtering.filter_streaks(img, sigma=SIGMA, level=5, route="march")
    with pytest.warns(UserWarning):
        a = filtering.filter_streaks(img, sigma=SIGMA, level=5, route="auto")
    with pytest.warns(UserWarning):
        b = filtering.filter_streaks(img, sigma=SIGMA, level=5, route="generic")
    assert np.array_equal(a, b)


def test_default_route_is_the_generic_one():
    img = mc.plane(4, 96, 128)
    a = filtering.filter_streaks(img, sigma=SIGMA)
    b = filtering.filter_streaks(img, sigma=SIGMA, route="generic")
    assert np.array_equal(a, b)
    pa = filtering.destripe_streaks_planes(img[None], SIGMA)
    pb = filtering.destripe_streaks_planes(img[None], SIGMA, route="generic")
    assert np.array_equal(pa, pb)
    m = filtering.filter_streaks(img, sigma=SIGMA, route="march")
    assert not np.array_equal(a, m)  # another chain: the same filter, other roundings


def test_float32_pixel_without_finite_log_raises():
    img = mc.plane(1, 64, 64, np.float32)
    img[10, 20] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        filtering.filter_streaks(img, sigma=SIGMA, threshold=300.0, route="march")
    filtering.filter_streaks(mc.plane(2, 64, 64, np.float32), sigma=SIGMA, threshold=300.0, route="march")


def test_stripe_plan_after_a_march_plan_on_the_same_engine():
    """A march plan holds a log-space plan of its own; the stripe plan that replaces it must not inherit anything."""
    planes = np.stack([mc.plane(k, 96, 128) for k in range(3)])
    fresh = eng_mod.DestripeEngine(0)
    used = eng_mod.DestripeEngine(0)
    try:
        fresh.plan(96, 128, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, 2700, max_batch=3)
        want, want_cfg = fresh.run(planes, out_dtype=np.float32, return_cfg=True)
        used.plan_streaks(96, 128, 8.0, 16.0, max_batch=3, route="march")
        m = used.run(planes, out_dtype=np.float32)
        used.plan(96, 128, synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, 2700, max_batch=3)
        got, got_cfg = used.run(planes, out_dtype=np.float32, return_cfg=True)
        assert np.array_equal(got, want) and np.array_equal(got_cfg, want_cfg)
        used.plan_streaks(96, 128, 8.0, 16.0, max_batch=3, route="march")
        assert np.array_equal(used.run(planes, out_dtype=np.float32), m)
    finally:
        fresh.close()
        used.close()
    # and through the engine cache of filtering: stripes after streaks equal stripes alone
    filtering.release_engines()
    a = filtering.destripe_planes(planes, "X_0_Y_0", no_cells_config=synth.NO_CELLS_CONFIG, cells_config=synth.CELLS_CONFIG)
    filtering.release_engines()
    filtering.destripe_streaks_planes(planes, SIGMA, route="march")
    b = filtering.destripe_planes(planes, "X_0_Y_0", no_cells_config=synth.NO_CELLS_CONFIG, cells_config=synth.CELLS_CONFIG)
    assert np.array_equal(a, b)
