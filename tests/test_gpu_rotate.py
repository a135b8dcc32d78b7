"""``rotate=True`` on the GPU: vertical stripes.  The contract is ``F(x, rotate=True) == np.rot90(F(np.rot90(x)), -1)``
per plane, with ``F`` the same call without the option.  A quarter turn is pure data movement, so the identity is held
byte for byte; one case ties the direction of the turn to the NumPy restatement of the dual-band filter
(tests/streaks_oracle.py) within the suite's standing ``1e-4 (1 + |ref|)``."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, engine, mini_tiff, pyramid, synth
from aind_smartspim_destripe_amd import filtering as fl
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from tests import streaks_oracle as so

pytestmark = pytest.mark.gpu

CELLS, NO_CELLS = synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG
SHAPES = [(1, 1), (1, 7), (3, 5), (63, 65), (64, 64), (70, 100), (129, 257)]
CANARY = 256  # bytes either side of the destination


def rot(a, k=1):
    """``np.rot90`` of every plane of ``a[..., H, W]``, contiguous."""
    return np.ascontiguousarray(np.rot90(a, k, axes=(-2, -1)))


def vertical_planes(n, H, W, dtype=np.uint16, first=0):
    """``[n, H, W]`` planes whose stripes run down the columns: turned, they are the suite's own striped planes."""
    return rot(np.stack([synth.synthetic_plane(first + k, W, H) for k in range(n)]), -1).astype(dtype)


# ---- 1. the kernel on its own -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = engine.DestripeEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_rot90_device_is_np_rot90(eng, dtype):
    rng = np.random.default_rng(7)
    for H, W in SHAPES:
        for n in (1, 3):
            x = (rng.integers(0, 65536, (n, H, W)).astype(dtype) if dtype == np.uint16
                 else rng.standard_normal((n, H, W)).astype(np.float32))  # fmt: skip
            d_src, d_dst = eng.alloc(max(x.nbytes, 16)), eng.alloc(x.nbytes + 2 * CANARY)
            try:
                d_src.upload(x)
                for direction in (1, -1):
                    d_dst.upload(np.full(x.nbytes + 2 * CANARY, 0xA5, np.uint8))
                    inner = engine.DeviceBuffer.__new__(engine.DeviceBuffer)  # the destination between the canaries
                    inner.engine, inner.ptr, inner.nbytes = eng, d_dst.ptr + CANARY, x.nbytes
                    eng.rot90_device(d_src, inner, dtype, n, H, W, direction)
                    eng.sync()
                    raw = d_dst.download((x.nbytes + 2 * CANARY,), np.uint8)
                    got = raw[CANARY : CANARY + x.nbytes].view(dtype).reshape(n, W, H)
                    assert got.tobytes() == rot(x, direction).tobytes(), (H, W, n, direction)
                    assert (raw[:CANARY] == 0xA5).all() and (raw[CANARY + x.nbytes :] == 0xA5).all(), (H, W, n, direction)
            finally:
                d_src.free()
                d_dst.free()
    d = eng.alloc(64)
    with pytest.raises(ValueError):
        eng.rot90_device(d, d, np.uint16, 1, 2, 3, 1)  # in place
    d.free()


# ---- 2. log-space filter ------------------------------------------------------------------------------------------
def _log_identity(x, out_dtype, max_batch=32, sc=None, sc_rot=None, cells=CELLS, no_cells=NO_CELLS):
    got, cfg = fl.destripe_planes(x, "X_0_Y_0", no_cells, cells, sc, synth.ZARR_PATH_HIGH_INT, out_dtype=out_dtype,
                                  max_batch=max_batch, return_config=True, rotate=True)  # fmt: skip
    ref, cfg_ref = fl.destripe_planes(rot(x), "X_0_Y_0", no_cells, cells, sc_rot, synth.ZARR_PATH_HIGH_INT,
                                      out_dtype=out_dtype, max_batch=max_batch, return_config=True)  # fmt: skip
    want = rot(ref, -1)
    H, W = x.shape[1:]
    assert got.shape == (x.shape[0], H + H % 2, W + W % 2) and got.dtype == np.dtype(out_dtype)
    assert got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(cfg, cfg_ref)
    return got


@pytest.mark.parametrize("shape,in_dtype", [((70, 100), np.uint16), ((70, 100), np.float32), ((101, 103), np.uint16),
                                            ((96, 128), np.uint16)],
                         ids=["70x100-u16", "70x100-f32", "101x103", "96x128"])  # fmt: skip
@pytest.mark.parametrize("out_dtype", [np.uint16, np.float32], ids=["to-u16", "to-f32"])
def test_log_space_identity(shape, in_dtype, out_dtype):
    x = vertical_planes(5, *shape, dtype=in_dtype)
    x[1] += in_dtype(3000)  # a bright plane: both configs are taken
    _log_identity(x, out_dtype, max_batch=2)  # 5 planes in cohorts of 2, 2, 1


def test_log_space_identity_one_cohort_of_many_parts():
    _log_identity(vertical_planes(9, 70, 100), np.uint16, max_batch=32)


def _shading(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.2 * ((yy / H - 0.4) ** 2 + (xx / W - 0.6) ** 2)).astype(np.float32)
    dark = (90.0 + 0.5 * np.arange((H + 10) * (W + 6)).reshape(H + 10, W + 6) % 17).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": dark}
    sc_rot = {"retrospective": True, "flatfield": rot(flat), "darkfield": rot(dark[:H, :W])}  # cropped, then turned
    return sc, sc_rot


def test_log_space_identity_with_flat_and_a_larger_dark():
    sc, sc_rot = _shading(70, 100)
    _log_identity(vertical_planes(3, 70, 100), np.uint16, sc=sc, sc_rot=sc_rot)
    _log_identity(vertical_planes(3, 70, 100), np.float32, sc=sc, sc_rot=sc_rot)


def test_filter_stripes_and_stack_mode():
    x = vertical_planes(3, 70, 100)
    got = fl.filter_stripes(x[0], "X_0_Y_0", NO_CELLS, CELLS, None, 2700, rotate=True)
    want = np.rot90(fl.filter_stripes(rot(x[0]), "X_0_Y_0", NO_CELLS, CELLS, None, 2700), -1)
    assert got.dtype == want.dtype == np.float64 and got.tobytes() == np.ascontiguousarray(want).tobytes()
    sc, sc_rot = _shading(70, 100)
    got = fl.filter_stripes(x[0], "X_0_Y_0", NO_CELLS, CELLS, sc, 2700, rotate=True)
    want = np.rot90(fl.filter_stripes(rot(x[0]), "X_0_Y_0", NO_CELLS, CELLS, sc_rot, 2700), -1)
    assert got.dtype == np.uint16 and got.tobytes() == np.ascontiguousarray(want).tobytes()
    # the 3-D stack mode: one Otsu threshold per level over all planes, each plane turned on its own
    got = fl.log_space_fft_filtering(x, level=3, sigma=64, rotate=True)
    want = rot(fl.log_space_fft_filtering(rot(x), level=3, sigma=64), -1)
    assert got.shape == x.shape and got.tobytes() == want.tobytes()
    got = fl.filter_streaks(x[0], sigma=64, level=2, rotate=True)  # the scalar form forwards
    want = rot(fl.log_space_fft_filtering(rot(x[0]), level=2, sigma=64), -1)
    assert got.tobytes() == want.tobytes()


def test_log_space_identity_other_wavelet():
    cells, no_cells = dict(CELLS, wavelet="sym4"), dict(NO_CELLS, wavelet="sym4")
    _log_identity(vertical_planes(3, 96, 128), np.uint16, cells=cells, no_cells=no_cells)
    # two wavelets: the statistic decides first, one engine per config
    x = vertical_planes(3, 96, 128)
    x[1] += np.uint16(3000)
    _log_identity(x, np.uint16, cells=dict(CELLS, wavelet="db2"), no_cells=NO_CELLS)


# ---- 3. dual-band filter ------------------------------------------------------------------------------------------
def _streaks_identity(x, sigma, out_dtype=np.uint16, flat=None, dark=None, **kw):
    got, t = fl.destripe_streaks_planes(x, sigma, out_dtype=out_dtype, return_threshold=True, rotate=True, flat=flat,
                                        dark=dark, **kw)  # fmt: skip
    H, W = x.shape[1:]
    rflat = None if flat is None else rot(flat)
    rdark = None if dark is None else rot(np.asarray(dark)[:H, :W])
    ref, t_ref = fl.destripe_streaks_planes(rot(x), sigma, out_dtype=out_dtype, return_threshold=True, flat=rflat,
                                            dark=rdark, **kw)  # fmt: skip
    assert got.shape == x.shape and got.tobytes() == rot(ref, -1).tobytes()
    np.testing.assert_array_equal(t, t_ref)
    return got


@pytest.mark.parametrize("route", ["generic", "march"])
def test_streaks_identity(route):
    x = vertical_planes(3, 64, 96)
    for out_dtype in (np.uint16, np.float32):
        _streaks_identity(x, (64, 128), out_dtype=out_dtype, route=route, max_batch=2)  # cohorts of 2 and 1
    _streaks_identity(x.astype(np.float32), (64, 128), out_dtype=np.float32, route=route, max_batch=2)
    sc, _ = _shading(64, 96)
    _streaks_identity(x, (64, 128), route=route, flat=sc["flatfield"], dark=sc["darkfield"])


def test_streaks_identity_options():
    x = vertical_planes(3, 64, 96)
    _streaks_identity(x, (64, None))
    _streaks_identity(x, (64, 128), smoothing=1)
    _streaks_identity(x, (64, 128), threshold=700, out_dtype=np.float32)


def test_streaks_identity_odd_plane():
    _streaks_identity(vertical_planes(2, 65, 99), (64, 128), out_dtype=np.float32)


def test_streaks_direction_is_the_written_one():
    """The anchor: the NumPy restatement on ``np.rot90(x)``, turned back with ``np.rot90(., -1)``."""
    x = vertical_planes(1, 64, 96)[0]
    t_ref, ref = so.filter_streaks(np.rot90(x), (64, 128))
    want = np.rot90(ref, -1)
    for route in ("generic", "march"):
        got, t = fl.destripe_streaks_planes(x[None], (64, 128), out_dtype=np.float32, return_threshold=True, route=route,
                                            rotate=True)  # fmt: skip
        assert t[0] == t_ref
        err = np.abs(got[0].astype(np.float64) - want) / (1 + np.abs(want))
        print("route {}: max error {:.3e} of 1e-4".format(route, err.max()))
        assert err.max() < 1e-4, (route, float(err.max()))
        pair = fl.filter_streaks(x, (64, 128), route=route, rotate=True)
        assert pair.tobytes() == got[0].astype(np.float64).tobytes()
    # the other direction is a different image: the planes are not symmetric under a half turn
    assert np.abs(np.rot90(ref, 1) - want).max() > 1


# ---- 4. cache keys, and a plain plan after a rotated one -----------------------------------------------------------
def test_rotated_and_plain_engines_side_by_side():
    x = vertical_planes(3, 70, 100)
    plain0 = fl.destripe_planes(x, "X_0_Y_0", NO_CELLS, CELLS, None, 2500)
    turned = fl.destripe_planes(x, "X_0_Y_0", NO_CELLS, CELLS, None, 2500, rotate=True)
    plain1 = fl.destripe_planes(x, "X_0_Y_0", NO_CELLS, CELLS, None, 2500)
    assert plain0.tobytes() == plain1.tobytes() != turned.tobytes()
    assert turned.tobytes() == rot(fl.destripe_planes(rot(x), "X_0_Y_0", NO_CELLS, CELLS, None, 2500), -1).tobytes()
    assert fl.get_engine((70, 100), CELLS, NO_CELLS, 2500) is not fl.get_engine((70, 100), CELLS, NO_CELLS, 2500, rotate=True)
    s0 = fl.destripe_streaks_planes(x, (64, 128))
    s1 = fl.destripe_streaks_planes(x, (64, 128), rotate=True)
    assert s0.tobytes() == fl.destripe_streaks_planes(x, (64, 128)).tobytes() != s1.tobytes()


def test_a_plain_plan_after_a_rotated_one_is_the_plain_plan():
    x = vertical_planes(5, 70, 100)
    fresh, e = engine.DestripeEngine(0), engine.DestripeEngine(0)
    try:
        info0 = fresh.plan(70, 100, CELLS, NO_CELLS, 2500, max_batch=4)
        want, want_cfg = fresh.run(x, out_dtype=np.uint16, return_cfg=True)
        info_r = e.plan(70, 100, CELLS, NO_CELLS, 2500, max_batch=4, rotate=True)
        assert (info_r.height, info_r.width, info_r.out_height, info_r.out_width) == (70, 100, 70, 100)
        assert e.level_shape(0) == (info0.level_w[0], info0.level_h[0])  # levels are those of the rotated chain
        turned = e.run(x, out_dtype=np.uint16)
        assert turned.tobytes() != want.tobytes()
        # the device-buffer path in the caller's orientation, twice in a row (the second call queues behind the first)
        d_in, d_out = e.alloc(x.nbytes), e.alloc(x.nbytes)
        d_in.upload(x)
        for _ in range(2):
            e.run_device(d_in, np.uint16, 4, d_out, np.uint16)
        e.sync()
        assert d_out.download((4, 70, 100), np.uint16).tobytes() == turned[:4].tobytes()
        d_in.free()
        d_out.free()
        info1 = e.plan(70, 100, CELLS, NO_CELLS, 2500, max_batch=4)
        assert info1.workspace_bytes == info0.workspace_bytes
        got, got_cfg = e.run(x, out_dtype=np.uint16, return_cfg=True)
        assert got.tobytes() == want.tobytes() and got_cfg.tobytes() == want_cfg.tobytes()
        assert e.info.workspace_bytes == info0.workspace_bytes
        info = engine._PlanInfo()
        e._check(e._lib.dsx_plan_info(e._ctx, info))
        assert info.workspace_bytes == info0.workspace_bytes  # no rotation buffer after the plain run
        # a plane too high for the row filter once turned
        with pytest.raises(engine.DsxError, match="DSX_ELIMIT"):
            e.plan(40000, 64, CELLS, NO_CELLS, 2500, max_batch=1, rotate=True)
    finally:
        fresh.close()
        e.close()


def test_set_shading_device_takes_the_callers_orientation():
    x = vertical_planes(2, 70, 100)
    sc, _ = _shading(70, 100)
    flat, dark = sc["flatfield"], sc["darkfield"]
    want = fl.destripe_planes(x, "X_0_Y_0", NO_CELLS, CELLS, sc, 2500, rotate=True)
    e = engine.DestripeEngine(0)
    try:
        e.plan(70, 100, CELLS, NO_CELLS, 2500, max_batch=2, rotate=True)
        d_flat, d_dark = e.alloc(flat.nbytes), e.alloc(dark.nbytes)
        d_flat.upload(flat)
        d_dark.upload(dark)
        e._check(e._lib.dsx_set_shading_device(e._ctx, d_flat.ptr, d_dark.ptr, *dark.shape))
        assert e.run(x, out_dtype=np.uint16).tobytes() == want.tobytes()
    finally:
        e.close()


# ---- 5. stores ----------------------------------------------------------------------------------------------------
Z, H, W, BRICK = 8, 96, 128, (1, 1, 4, 32, 32)


@pytest.fixture(scope="module")
def volume():
    vol = vertical_planes(Z, H, W)
    want = fl.destripe_planes(vol, "X_0_Y_0", NO_CELLS, CELLS, None, synth.ZARR_PATH_HIGH_INT, rotate=True)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def _store(tmp_path, vol, compressor):
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1) + vol.shape, BRICK, np.uint16, compressor=compressor)
    src[0, 0] = vol
    return path


def test_store_raw_chunks_device_retile(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, None)
    try:
        out = str(tmp_path / "out" / "0")
        n, _ = zd.destripe_zarr_store(src, out, CELLS, NO_CELLS, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                                      device=0, compressor=None, device_retile=True, rotate=True)  # fmt: skip
        assert n == Z and zd.LAST_RUN["rotate"] is True
        assert MiniZarrArray.open(out)[0, 0].tobytes() == want.tobytes()
        # the dual-band filter through the same store, the option in the dict
        out = str(tmp_path / "out_streaks" / "0")
        n, _ = zd.destripe_zarr_store(src, out, None, None, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                                      device=0, compressor=None, device_retile=True,
                                      streaks={"sigma": (64, 128), "rotate": True})  # fmt: skip
        assert n == Z and zd.LAST_RUN["rotate"] is True and zd.LAST_RUN["filter"] == "streaks"
        ref = fl.destripe_streaks_planes(vol, (64, 128), rotate=True, route=zd.LAST_RUN["streaks_route"])
        assert MiniZarrArray.open(out)[0, 0].tobytes() == ref.tobytes()
        # and off again: today's store
        out = str(tmp_path / "out_plain" / "0")
        zd.destripe_zarr_store(src, out, CELLS, NO_CELLS, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                               device=0, compressor=None, device_retile=True)  # fmt: skip
        assert zd.LAST_RUN["rotate"] is False
        plain = fl.destripe_planes(vol, "X_0_Y_0", NO_CELLS, CELLS, None, synth.ZARR_PATH_HIGH_INT)
        assert MiniZarrArray.open(out)[0, 0].tobytes() == plain.tobytes()
    finally:
        zd.release_staging()


def test_store_device_codecs_pyramid_and_histogram(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, "blosc")
    hist = np.zeros(engine.VOLHIST_BINS, np.int64)
    group = str(tmp_path / "out")
    try:
        n, _ = zd.destripe_zarr_store(src, os.path.join(group, "0"), CELLS, NO_CELLS, None, prediction_chunksize=(8, H, W),
                                      output_chunks=BRICK, device=0, compressor="blosc", device_retile=True,
                                      device_codec="runs", device_decode=True, pyramid_group=group, n_levels=3,
                                      histogram=hist, rotate=True)  # fmt: skip
    finally:
        zd.release_staging()
    assert n == Z and zd.LAST_RUN["rotate"] is True and zd.LAST_RUN["pyramid_levels"] == [1, 2]
    assert zd.LAST_RUN["device_codec_mode"] == "runs" and zd.LAST_RUN["device_decode"] is True
    level0 = MiniZarrArray.open(os.path.join(group, "0"))[0, 0]
    assert level0.tobytes() == want.tobytes()
    np.testing.assert_array_equal(hist, np.bincount(want.ravel(), minlength=engine.VOLHIST_BINS))
    ref_group = str(tmp_path / "ref")
    pyramid.write_pyramid_levels(os.path.join(group, "0"), ref_group, n_levels=3, chunks=BRICK, compressor="blosc", device=0)
    for lvl in (1, 2):
        a = MiniZarrArray.open(os.path.join(group, str(lvl)))
        b = MiniZarrArray.open(os.path.join(ref_group, str(lvl)))
        assert a.shape == b.shape and a.chunks == b.chunks and a[0, 0].tobytes() == b[0, 0].tobytes(), lvl


def test_store_host_path(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, "blosc")
    out = str(tmp_path / "out" / "0")
    n, _ = zd.destripe_zarr_store(src, out, CELLS, NO_CELLS, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                                  device=0, compressor="blosc", device_retile=False, rotate=True)  # fmt: skip
    assert n == Z and zd.LAST_RUN["rotate"] is True
    assert MiniZarrArray.open(out)[0, 0].tobytes() == want.tobytes()


# ---- 6. directory mode --------------------------------------------------------------------------------------------
def test_batch_filter_rotate(tmp_path):
    x = vertical_planes(3, 70, 100)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for k in range(3):
        mini_tiff.imwrite(str(src / "plane_{}.tif".format(k)), x[k])
    n = destriper.batch_filter(src, dst, 2, 4, CELLS, NO_CELLS, None, rotate=True)
    assert n == 3
    for k in range(3):
        want = fl.filter_stripes(x[k], str(src / "plane_{}.tif".format(k)), NO_CELLS, CELLS, None, rotate=True).astype(np.uint16)
        got = mini_tiff.imread(str(dst / "plane_{}.tiff".format(k)))
        assert got.tobytes() == want.tobytes(), k
    destriper.read_filter_save(dst, src / "plane_0.tif", dst / "single.tif", CELLS, NO_CELLS, rotate=True)
    want = fl.filter_stripes(x[0], "p", NO_CELLS, CELLS, None, rotate=True).astype(np.uint16)
    assert mini_tiff.imread(str(dst / "single.tiff")).tobytes() == want.tobytes()
