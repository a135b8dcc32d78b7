"""The light-sheet background mode on the GPU (``dsx_plan_lightsheet``; ``csrc/dsx_lightsheet.h``) against its host
build (``engine.lightsheet_ref``, which ``test_lightsheet_host.py`` ties to scikit-image's ``rank.percentile``) on every
case of ``lightsheet_cases``.  Every step is integer or a single float32 operation, so everything is held byte for
byte."""

import functools
import os

import numpy as np
import pytest

import lightsheet_cases as lc
from aind_smartspim_destripe_amd import destriper, engine, mini_tiff
from aind_smartspim_destripe_amd import filtering as fl
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

CASES = {name: (x, prm) for name, x, prm in lc.cases()}
OPTS = dict(artifact_length=15, background_window_size=20)  # the small windows of the batch / pipeline tests


@functools.lru_cache(maxsize=None)
def host(name):
    x, prm = CASES[name]
    out, ls, bg = engine.lightsheet_ref(x, **prm)
    for a in (out, ls, bg):
        a.setflags(write=False)
    return out, ls, bg


def host_planes(planes, **prm):
    return np.stack([engine.lightsheet_ref(p, out_dtype=np.uint16, **prm)[0] for p in planes])


@pytest.mark.parametrize("name", lc.case_names())
def test_device_is_the_host_build(name):
    x, prm = CASES[name]
    out, ls, bg = host(name)
    eng = engine.DestripeEngine(0)
    try:
        eng.plan_lightsheet(x.shape[0], x.shape[1], max_batch=1, **prm)
        got = eng.run(x[None], out_dtype=np.float32)[0]
        d_ls, d_bg = eng.lightsheet_planes(0)
        assert d_ls.tobytes() == ls.tobytes()
        assert d_bg.tobytes() == bg.tobytes()
        assert got.dtype == np.float32 and got.tobytes() == out.tobytes()
        u16 = eng.run(x[None], out_dtype=np.uint16)[0]
        assert u16.dtype == np.uint16 and u16.tobytes() == out.astype(np.uint16).tobytes()
        with pytest.raises(engine.DsxError):  # uint16 in only
            eng.run(x[None].astype(np.float32), out_dtype=np.float32)
    finally:
        eng.close()
    assert fl.correct_lightsheet(x, **prm).tobytes() == out.tobytes()


def test_batch_of_five_in_cohorts_of_two():
    planes = np.stack([lc.glow_plane(20 + k, 70, 100) for k in range(5)])
    want = host_planes(planes, **OPTS)
    got = fl.correct_lightsheet_planes(planes, max_batch=2, **OPTS)
    assert got.dtype == np.uint16 and got.tobytes() == want.tobytes()
    for k in range(5):
        assert fl.correct_lightsheet(planes[k], **OPTS).astype(np.uint16).tobytes() == want[k].tobytes(), k
    f32 = fl.correct_lightsheet_planes(planes, max_batch=2, out_dtype=np.float32, **OPTS)
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.uint16), want)


@pytest.mark.parametrize("shape", [(70, 100), (37, 53)])
def test_rotate_is_rot90_around_the_plain_call(shape):
    x = lc.glow_plane(30, *shape)
    prm = dict(artifact_length=31, background_window_size=24)
    plain = fl.correct_lightsheet(np.ascontiguousarray(np.rot90(x)), **prm)
    got = fl.correct_lightsheet(x, rotate=True, **prm)
    assert got.shape == x.shape and got.tobytes() == np.ascontiguousarray(np.rot90(plain, -1)).tobytes()
    assert got.tobytes() != fl.correct_lightsheet(x, **prm).tobytes()  # (the turn does something on these planes)
    stack = np.stack([x, lc.glow_plane(31, *shape), lc.glow_plane(32, *shape)])
    both = fl.correct_lightsheet_planes(stack, rotate=True, max_batch=2, **prm)
    assert both[0].tobytes() == got.astype(np.uint16).tobytes()
    assert both[2].tobytes() == fl.correct_lightsheet(stack[2], rotate=True, **prm).astype(np.uint16).tobytes()


def test_batch_filter_lightsheet(tmp_path):
    x = np.stack([lc.glow_plane(40 + k, 70, 100) for k in range(3)])
    want = host_planes(x, **OPTS)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for k in range(3):
        mini_tiff.imwrite(str(src / "plane_{}.tif".format(k)), x[k])
    assert destriper.batch_filter(src, dst, 2, 2, None, None, None, lightsheet=OPTS) == 3
    for k in range(3):
        assert mini_tiff.imread(str(dst / "plane_{}.tiff".format(k))).tobytes() == want[k].tobytes(), k
    destriper.read_filter_save(dst, src / "plane_1.tif", dst / "single.tif", None, None, lightsheet=OPTS)
    assert mini_tiff.imread(str(dst / "single.tiff")).tobytes() == want[1].tobytes()


Z, H, W, BRICK = 8, 96, 128, (1, 1, 4, 32, 32)


@pytest.fixture(scope="module")
def volume():
    vol = np.stack([lc.glow_plane(50 + k, H, W) for k in range(Z)])
    want = host_planes(vol, **OPTS)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def _store(tmp_path, vol, compressor):
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1) + vol.shape, BRICK, np.uint16, compressor=compressor)
    src[0, 0] = vol
    return path


def test_store_raw_chunks(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, None)
    out = str(tmp_path / "out" / "0")
    try:
        n, _ = zd.destripe_zarr_store(src, out, None, None, None, prediction_chunksize=(4, H, W), output_chunks=BRICK,
                                      device=0, compressor=None, device_retile=True, lightsheet=OPTS)  # fmt: skip
    finally:
        zd.release_staging()
    assert n == Z and zd.LAST_RUN["filter"] == "lightsheet" and zd.LAST_RUN["streaks_route"] is None
    assert MiniZarrArray.open(out)[0, 0].tobytes() == want.tobytes()
    # the host path writes the same store
    out = str(tmp_path / "out_host" / "0")
    n, _ = zd.destripe_zarr_store(src, out, None, None, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                                  device=0, compressor=None, device_retile=False, lightsheet=OPTS)  # fmt: skip
    assert n == Z and zd.LAST_RUN["filter"] == "lightsheet"
    assert MiniZarrArray.open(out)[0, 0].tobytes() == want.tobytes()


def test_store_blosc_device_codecs(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, "blosc")
    out = str(tmp_path / "out" / "0")
    try:
        n, _ = zd.destripe_zarr_store(src, out, None, None, None, prediction_chunksize=(8, H, W), output_chunks=BRICK,
                                      device=0, compressor="blosc", device_retile=True, device_codec="runs",
                                      device_decode=True, lightsheet=OPTS)  # fmt: skip
    finally:
        zd.release_staging()
    assert n == Z and zd.LAST_RUN["filter"] == "lightsheet"
    assert zd.LAST_RUN["device_codec_mode"] == "runs" and zd.LAST_RUN["device_decode"] is True
    assert MiniZarrArray.open(out)[0, 0].tobytes() == want.tobytes()


def test_destripe_zarr_lightsheet(tmp_path, volume):
    vol, want = volume
    src = _store(tmp_path, vol, "blosc")
    out = tmp_path / "results" / "X_0_Y_0.zarr"
    try:
        n, _ = zd.destripe_zarr(dataset_path=src, multiscale="0", output_destriped_zarr=str(out),
                                prediction_chunksize=(8, H, W), parameters={}, n_workers=1, batch_size=1,
                                super_chunksize=None, target_size_mb=1, results_folder=str(tmp_path / "results"),
                                xyz_resolution=[1.0, 1.0, 1.0], derivatives_path=str(tmp_path / "none"), flatfield=None,
                                output_chunks=BRICK, n_levels=1, lightsheet=OPTS)  # fmt: skip
    finally:
        zd.release_staging()
    assert n == Z and zd.LAST_RUN["filter"] == "lightsheet"
    assert MiniZarrArray.open(os.path.join(str(out), "0"))[0, 0].tobytes() == want.tobytes()
