"""GPU: the dual-band filter through the pipelines (``streaks=`` of ``destripe_zarr_store``, ``destripe_zarr`` and
``batch_filter``).  Every voxel of an output equals ``destripe_streaks_planes`` of the input planes on the same route.
Store geometry: 12 planes of 64 x 96 in (4, 32, 32) chunks, z blocks of 4 planes -- three blocks, so both staging
buffer sets are used twice."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, filtering, mini_tiff, pyramid
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from tests import streaks_march_cases as mc

pytestmark = pytest.mark.gpu

Z, H, W = 12, 64, 96
CHUNKS = (1, 1, 4, 32, 32)
SIGMA = (8.0, 16.0)
LZ4 = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


@pytest.fixture(scope="module")
def volume():
    vol = np.stack([mc.plane(300 + k, H, W) for k in range(Z)])
    vol.setflags(write=False)
    return vol


@pytest.fixture(scope="module")
def expected(volume):
    """The filter's own answer per route, computed once."""
    out = {r: filtering.destripe_streaks_planes(volume, SIGMA, route=r, out_dtype=np.uint16) for r in ("generic", "march")}
    for a in out.values():
        a.setflags(write=False)
    return out


def _input(tmp_path, volume, compressor):
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, Z, H, W), CHUNKS, np.uint16, compressor=compressor)
    src[0, 0] = volume
    return path


def _store(in_path, out, route, compressor, **kw):
    n, _ = zd.destripe_zarr_store(in_path, out, None, None, None, prediction_chunksize=(4, H, W), output_chunks=CHUNKS,
                                  device=0, compressor=compressor, io_threads=4,
                                  streaks={"sigma": SIGMA, "route": route}, **kw)  # fmt: skip
    assert n == Z
    assert zd.LAST_RUN["filter"] == "streaks" and zd.LAST_RUN["streaks_route"] == route
    return MiniZarrArray.open(out)[0, 0]


@pytest.mark.parametrize("route", ["generic", "march"])
def test_store_voxels_are_the_filters(tmp_path, volume, expected, route):
    try:
        raw = _input(tmp_path, volume, None)
        got = _store(raw, str(tmp_path / "raw_out"), route, None, device_retile=True)
        assert np.array_equal(got, expected[route])
        got = _store(raw, str(tmp_path / "host_out"), route, None, device_retile=False)
        assert np.array_equal(got, expected[route])

        blosc = tmp_path / "blosc"
        blosc.mkdir()
        zin = _input(blosc, volume, "blosc")
        g = str(blosc / "group")
        got = _store(zin, os.path.join(g, "0"), route, "blosc", device_retile=True, device_codec="runs",
                     device_decode=True, pyramid_group=g, n_levels=2)  # fmt: skip
        assert zd.LAST_RUN["device_codec_mode"] == "runs" and zd.LAST_RUN["pyramid_levels"] == [1]
        assert np.array_equal(got, expected[route])
        two = str(blosc / "two_pass")  # the levels write_pyramid_levels makes of that level 0
        pyramid.write_pyramid_levels(os.path.join(g, "0"), two, n_levels=2, chunks=CHUNKS, compressor="blosc")
        assert np.array_equal(MiniZarrArray.open(os.path.join(g, "1"))[0, 0], MiniZarrArray.open(os.path.join(two, "1"))[0, 0])

        got = _store(zin, str(blosc / "lz4_out"), route, LZ4, device_retile=True, device_codec=True)
        assert zd.LAST_RUN["device_codec_mode"] == "lz4"
        assert np.array_equal(got, expected[route])
    finally:
        zd.release_staging()


def test_stripe_runs_report_their_filter(tmp_path, volume):
    from aind_smartspim_destripe_amd import synth

    try:
        zd.destripe_zarr_store(_input(tmp_path, volume, None), str(tmp_path / "o"), synth.CELLS_CONFIG,
                               synth.NO_CELLS_CONFIG, None, prediction_chunksize=(4, H, W), output_chunks=CHUNKS, device=0,
                               compressor=None, io_threads=4)  # fmt: skip
        assert zd.LAST_RUN["filter"] == "stripes" and zd.LAST_RUN["streaks_route"] is None
    finally:
        zd.release_staging()


@pytest.mark.parametrize("route", ["generic", "march"])
def test_destripe_zarr_with_streaks(tmp_path, volume, expected, route):
    in_path = _input(tmp_path, volume, "blosc")
    group = str(tmp_path / "destriped" / "X_0_Y_0.zarr")
    try:
        n, _ = zd.destripe_zarr(in_path, "0", group, (4, H, W), 0, 1, 1, None, str(tmp_path / "results"),
                                str(tmp_path / "no_derivatives"), None, {}, device=0, output_chunks=CHUNKS, n_levels=2,
                                io_threads=4, streaks={"sigma": SIGMA, "route": route})  # fmt: skip
        assert n == Z and zd.LAST_RUN["filter"] == "streaks" and zd.LAST_RUN["streaks_route"] == route
        assert np.array_equal(MiniZarrArray.open(os.path.join(group, "0"))[0, 0], expected[route])
        assert MiniZarrArray.open(os.path.join(group, "1")).shape[-3:] == (Z // 2, H // 2, W // 2)
    finally:
        zd.release_staging()


def test_batch_filter_with_streaks(tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out"
    (src / "b").mkdir(parents=True)
    dst.mkdir()
    planes = {os.path.join("", "p{}.tiff".format(k)): mc.plane(400 + k, 64, 96) for k in range(3)}
    planes[os.path.join("b", "q.tiff")] = mc.plane(410, 96, 128)
    for name, img in planes.items():
        mini_tiff.imwrite(str(src / name), img)
    n = destriper.batch_filter(src, dst, 2, 4, None, None, None, streaks={"sigma": SIGMA})
    assert n == 4
    one = tmp_path / "one"
    one.mkdir()
    for name, img in planes.items():
        want = filtering.destripe_streaks_planes(img[None], SIGMA, route="auto", out_dtype=np.uint16)[0]
        got = mini_tiff.imread(str(dst / name))
        assert got.dtype == np.uint16 and np.array_equal(got, want), name
    # read_filter_save: one plane through filter_streaks, then the cast of the stripe path (astype to the source dtype)
    img = planes["p0.tiff"]
    destriper.read_filter_save(one, src / "p0.tiff", one / "p0.tiff", None, None, None, streaks={"sigma": SIGMA})
    want = filtering.filter_streaks(img, sigma=SIGMA, route="auto").astype(np.uint16)
    got = mini_tiff.imread(str(one / "p0.tiff"))
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(got, mini_tiff.imread(str(dst / "p0.tiff")))  # in range: the same as batch_filter's clip
