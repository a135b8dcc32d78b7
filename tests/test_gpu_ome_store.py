"""The histogram of the written voxels (``destripe_zarr_store(histogram=...)``) against the store it describes, and the
OME-NGFF metadata of the three pyramid routes of ``destripe_zarr`` with the window taken from it.  A 12 x 64 x 96
Blosc input in blocks of 4 planes: three blocks use both buffer sets and accumulate across blocks."""

import json
import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import mini_tiff, synth
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

Z, H, W = 12, 64, 96
CHUNKS = (1, 1, 4, 32, 32)
PARAMS = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
XYZ = (1.8, 1.9, 2.0)  # x, y, z as run_capsule hands them over


def _make_input(folder, width=W):
    path = str(folder / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(os.path.join(path, "0"), (1, 1, Z, H, width), CHUNKS, np.uint16, compressor="blosc")
    src[0, 0] = synth.synthetic_stack(Z, H, width, n_unique=4)
    return path


@pytest.fixture(scope="module")
def tile(tmp_path_factory):
    return _make_input(tmp_path_factory.mktemp("ome_in"))


@pytest.fixture(autouse=True)
def _release():
    yield
    zd.release_staging()


def _store(src, out, **kw):
    return zd.destripe_zarr_store(os.path.join(src, "0"), os.path.join(out, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                  None, prediction_chunksize=(4, H, kw.pop("width", W)), output_chunks=CHUNKS, device=0,
                                  io_threads=4, **kw)  # fmt: skip


def _level0(out):
    return MiniZarrArray.open(os.path.join(out, "0"))[0, 0]


@pytest.mark.parametrize("name,kw", [
    ("stripes", dict(device_retile=True)),
    ("streaks", dict(device_retile=True, streaks={"sigma": (8.0, 16.0)})),
    ("device_codecs", dict(device_retile=True, device_codec="runs", device_decode=True)),
])  # fmt: skip
def test_store_histogram_is_the_bincount_of_level_0(tmp_path, tile, name, kw):
    out = str(tmp_path / "out.zarr")
    h = np.zeros(65536, np.int64)
    n, _ = _store(tile, out, histogram=h, **kw)
    vol = _level0(out)
    assert n == Z and vol.shape == (Z, H, W)
    assert int(h.sum()) == Z * H * W == zd.LAST_RUN["histogram_voxels"]
    assert np.array_equal(h, np.bincount(vol.ravel(), minlength=65536))
    again = h.copy()
    _store(tile, out, histogram=again, **kw)  # the call ADDS to what it is given, from a freshly reset device histogram
    assert np.array_equal(again, 2 * h)


def test_store_histogram_on_the_host_route(tmp_path):
    """A 64 x 95 store cannot take the device re-tiling: the chunk map counts what ``execute_worker`` assigns."""
    src = _make_input(tmp_path, width=95)
    out = str(tmp_path / "out.zarr")
    h = np.zeros(65536, np.int64)
    n, _ = _store(src, out, histogram=h, width=95)
    vol = _level0(out)
    assert n == Z and vol.shape == (Z, H, 95)
    assert int(h.sum()) == Z * H * 95 == zd.LAST_RUN["histogram_voxels"]
    assert np.array_equal(h, np.bincount(vol.ravel(), minlength=65536))


def _files(path):
    out = {}
    for d, _, fs in os.walk(path):
        for f in fs:
            if f not in (".zattrs", ".zgroup"):
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), path)] = fh.read()
    return out


def _destripe_zarr(src, out, **kw):
    return zd.destripe_zarr(src, "0", out, (4, H, W), 3072, 0, 1, (Z, H, W), os.path.dirname(out),
                            os.path.join(os.path.dirname(out), "no_derivatives"), XYZ, PARAMS, device=0,
                            output_chunks=CHUNKS, n_levels=3, io_threads=4, device_retile=True, **kw)  # fmt: skip


def _attrs(group):
    with open(os.path.join(group, ".zattrs")) as f:
        return json.load(f)


def test_three_routes_write_the_same_metadata_and_the_same_arrays(tmp_path, tile):
    routes = {"two_pass": {}, "fused": dict(fused_pyramid=True), "pipelined": dict(pipelined_pyramid=True)}
    attrs = {}
    for name, kw in routes.items():
        plain = str(tmp_path / (name + "_plain") / "X_0_Y_0.zarr")
        with_md = str(tmp_path / (name + "_ome") / "X_0_Y_0.zarr")
        _destripe_zarr(tile, plain, **kw)
        # 3. options off: no metadata files, no histogram
        assert not os.path.exists(os.path.join(plain, ".zattrs")) and not os.path.exists(os.path.join(plain, ".zgroup"))
        assert zd.LAST_RUN["histogram_voxels"] is None and zd.LAST_RUN["display_window"] is None
        n, _ = _destripe_zarr(tile, with_md, ome_metadata=True, display_window="percentile", **kw)
        assert n == Z and zd.LAST_RUN["histogram_voxels"] == Z * H * W
        with open(os.path.join(with_md, ".zgroup")) as f:
            assert json.load(f) == {"zarr_format": 2}
        attrs[name] = _attrs(with_md)
        # the arrays are byte for byte those of the call without the options: .zarray and every chunk file
        a, b = _files(plain), _files(with_md)
        assert sorted(a) == sorted(b) and all(k.split(os.sep)[0] in "012" for k in a), name
        assert [k for k in a if a[k] != b[k]] == [], name
        vol = _level0(with_md)
        lo, hi = (float(v) for v in np.percentile(vol, (0.1, 95), method="lower"))
        want = (lo, max(hi, lo + 1.0))
        window = attrs[name]["omero"]["channels"][0]["window"]
        assert (window["start"], window["end"]) == want == tuple(zd.LAST_RUN["display_window"]), name
        assert (window["min"], window["max"]) == (0.0, 65535.0)
    assert attrs["two_pass"] == attrs["fused"] == attrs["pipelined"]
    md = attrs["fused"]
    assert md["omero"]["name"] == "X_0_Y_0.zarr" and md["omero"]["channels"][0]["label"] == "X_0_Y_0.zarr"
    assert md["omero"]["channels"][0]["color"] == "690afe" and md["omero"]["rdefs"]["defaultZ"] == Z // 2
    ms = md["multiscales"][0]
    assert [d["path"] for d in ms["datasets"]] == ["0", "1", "2"]
    z, y, x = XYZ[2], XYZ[1], XYZ[0]
    for lvl, d in enumerate(ms["datasets"]):  # the scales carry xyz_resolution in z, y, x order
        assert d["coordinateTransformations"] == [{"type": "scale", "scale": [1.0, 1.0, z * 2**lvl, y * 2**lvl, x * 2**lvl]}]
    assert [a["name"] for a in ms["axes"]] == list("tczyx") and ms["version"] == "0.4"


def test_fixed_windows_and_a_single_level(tmp_path, tile):
    out = str(tmp_path / "a" / "X_0_Y_0.zarr")
    _destripe_zarr(tile, out, ome_metadata=True, display_window=(5, 900.5))
    w = _attrs(out)["omero"]["channels"][0]["window"]
    assert (w["start"], w["end"]) == (5.0, 900.5) == tuple(zd.LAST_RUN["display_window"])
    assert zd.LAST_RUN["histogram_voxels"] is None  # a fixed window needs no histogram
    one = str(tmp_path / "b" / "X_0_Y_0.zarr")
    zd.destripe_zarr(tile, "0", one, (4, H, W), 3072, 0, 1, (Z, H, W), str(tmp_path / "b"), str(tmp_path / "none"), XYZ,
                     PARAMS, device=0, output_chunks=CHUNKS, n_levels=1, io_threads=4, ome_metadata=True)  # fmt: skip
    md = _attrs(one)
    assert [d["path"] for d in md["multiscales"][0]["datasets"]] == ["0"]  # compute_multiscale is not called: still written
    w = md["omero"]["channels"][0]["window"]
    assert (w["start"], w["end"]) == (0.0, 350.0)


def test_destripe_channel_writes_the_metadata_of_every_tile(tmp_path):
    chan = tmp_path / "data" / "Ex_488_Em_525"
    tiles = {"431040_368180": 0, "431040_394100": 1}
    for t, name in enumerate(tiles):
        a = MiniZarrArray.create(str(chan / (name + ".zarr") / "0"), (1, 1, Z, H, W), CHUNKS, np.uint16, compressor="blosc")
        a[0, 0] = synth.synthetic_stack(Z, H, W, n_unique=4) + np.uint16(t)
    d = tmp_path / "derivatives"
    d.mkdir()
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), np.full((H + 8, W + 8), 90, np.uint16))
    yy, xx = np.mgrid[0:H, 0:W]
    flats = {}
    for side in (0, 1):
        f = (1.0 + 0.2 * side - 0.3 * ((yy - H / 2) / H) ** 2 - 0.2 * ((xx - W / 2) / W) ** 2).astype(np.float32)
        flats[side] = str(d / "flat_{}.tif".format(side))
        mini_tiff.imwrite(flats[side], f)
    results = tmp_path / "results"
    done = zd.destripe_channel(str(tmp_path / "data"), str(d), "Ex_488_Em_525", str(results), XYZ, flats,
                               {side: [name for name, s in tiles.items() if s == side] for side in (0, 1)}, PARAMS,
                               prediction_chunksize=(4, H, W), output_chunks=CHUNKS, device=0, io_threads=4,
                               ome_metadata=True)  # fmt: skip
    assert done == {name + ".zarr": Z for name in tiles}
    for name in tiles:
        group = str(results / "destriped_data" / "Ex_488_Em_525" / (name + ".zarr"))
        with open(os.path.join(group, ".zgroup")) as f:
            assert json.load(f) == {"zarr_format": 2}
        md = _attrs(group)
        w = md["omero"]["channels"][0]["window"]
        assert (w["start"], w["end"], w["min"], w["max"]) == (0.0, 350.0, 0.0, 65535.0)
        assert md["omero"]["name"] == name + ".zarr"
        assert md["multiscales"][0]["datasets"][1]["coordinateTransformations"][0]["scale"] == [1.0, 1.0, 4.0, 3.8, 3.6]
        assert sorted(p for p in os.listdir(group) if not p.startswith(".")) == ["0", "1", "2"]
