"""GPU: the options of the dual-band filter (one-sided bands, a smoothed blend weight, dark / flat) on both routes,
against the real-library fixture ``tests/golden/streaks_options.npz``, and through the Zarr pipelines.
Bound: |gpu - ref| <= 1e-4 (1 + |ref|) on every pixel of the float32 output, ``t`` equal to the fixture's."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import filtering, mini_tiff
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from tests import streaks_options_oracle as soo

pytestmark = pytest.mark.gpu

BY_NAME = {c["name"]: c for c in soo.golden_cases()}
# (case, routes): the march route takes db3 and even planes
RUNS = [
    ("u16_64x96_smooth1", ("generic", "march")),
    ("u16_64x96_fg", ("generic", "march")),
    ("u16_64x96_bg", ("generic", "march")),
    ("u16_64x96_fg_smooth1", ("generic", "march")),
    ("u16_64x96_smooth1_shaded", ("generic", "march")),
    ("u16_33x47_sym4_smooth1_shaded", ("generic",)),
    ("u16_20x6_haar_smooth2", ("generic",)),
    ("f32_64x96_fg_fixed_t", ("generic", "march")),
]
PARAMS = [pytest.param(name, route, id="{}-{}".format(name, route)) for name, routes in RUNS for route in routes]
# Shading without smoothing is held to the fixture through the uint16 output only.  Where r is within a count of the dark
# plane, (r - dark) / flat turns the bands' float32 error (r is ~100 there, so a few ulp are ~1e-5) into an error of
# the order of 1e-4 (1 + |ref|) or more: measured 1.30e-4 on the generic route, one pixel of ref = 0.115.  The float
# epilogue of that case is checked on its own, to float32 rounding (test_shading_epilogue_alone).
PARAMS_U16 = PARAMS + [pytest.param("u16_64x96_shaded", r, id="u16_64x96_shaded-" + r) for r in ("generic", "march")]


def _run(case, route, out_dtype, **more):
    return filtering.destripe_streaks_planes(case["image"][None], route=route, out_dtype=out_dtype,
                                             **dict(soo.case_kwargs(case), **more))  # fmt: skip


@pytest.mark.parametrize("name,route", PARAMS)
def test_golden_case(name, route):
    case = BY_NAME[name]
    out, t = _run(case, route, np.float32, return_threshold=True)
    assert out.dtype == np.float32 and out.shape == (1,) + case["image"].shape
    assert t[0] == case["t"]
    ref = case["out"]
    err = np.abs(out[0].astype(np.float64) - ref) / (1.0 + np.abs(ref))
    print(name, route, "max err / (1 + |ref|) =", float(err.max()))
    assert np.all(err <= 1e-4), float(err.max())


@pytest.mark.parametrize("route", ["generic", "march"])
def test_shading_epilogue_alone(route):
    """Both bands, no smoothing: the shaded float32 output is flatfield_correction of the blend result r.  r is read
    from the same kernel with a flat of 1 and a dark of 0, which leave 0 <= r <= 65535 as it is, bit for bit; the blend
    before the epilogue is the same instruction sequence in both calls, so the two differ by the rounding of one float32
    subtraction and one division: 2 ulp of the result are allowed."""
    case = BY_NAME["u16_64x96_shaded"]
    shape = case["image"].shape
    r = _run(dict(case, flat=np.ones(shape, np.float32), dark=np.zeros(shape, np.float32)), route, np.float32)[0]
    assert r.min() > 0 and r.max() < 65535
    got = _run(case, route, np.float32)[0]
    dark = case["dark"][: r.shape[0], : r.shape[1]]
    want = np.clip(np.where(r > dark, r - dark, np.float32(0)) / case["flat"], 0, 65535).astype(np.float32)
    assert want.dtype == np.float32 and want.max() > 1000 and want.min() < 1
    assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)))


@pytest.mark.parametrize("name,route", PARAMS_U16)
def test_uint16_output(name, route):
    """uint16 is clip + truncate of the same call's float32 output exactly, and within one count of the fixture's."""
    case = BY_NAME[name]
    f = _run(case, route, np.float32)
    u = _run(case, route, np.uint16)
    assert u.dtype == np.uint16
    assert np.array_equal(u, np.clip(f, 0, 65535).astype(np.uint16))
    assert case["out"].max() < 9000  # 1e-4 (1 + v) stays below one count
    assert np.abs(u[0].astype(np.int64) - case["out_u16"].astype(np.int64)).max() <= 1


def test_shaded_float_output_is_the_clipped_value():
    case = BY_NAME["u16_64x96_shaded"]
    big = dict(case, image=(case["image"].astype(np.uint32) * 60).clip(0, 65535).astype(np.uint16))
    f = _run(big, "generic", np.float32)[0]
    _, ref = soo.filter_streaks(big["image"], big["sigma"], smoothing=big["smoothing"], flat=big["flat"], dark=big["dark"])
    assert ref.max() == 65535.0 and ref.min() >= 0.0 and np.any(ref % 1 != 0)  # clipped above, not truncated
    assert f.max() == 65535.0 and f.min() >= 0.0
    assert np.all(np.abs(f - ref) <= 1e-4 * (1 + np.abs(ref)))


def test_filter_streaks_returns_uint16_with_a_flat():
    case = BY_NAME["u16_64x96_smooth1_shaded"]
    out = filtering.filter_streaks(case["image"], **soo.case_kwargs(case))
    assert out.dtype == np.uint16 and out.shape == case["image"].shape
    assert np.abs(out.astype(np.int64) - case["out_u16"].astype(np.int64)).max() <= 1
    plain = BY_NAME["u16_64x96_fg_smooth1"]
    out = filtering.filter_streaks(plain["image"], **soo.case_kwargs(plain))
    assert out.dtype == np.float64


def test_equal_sigmas_take_smoothing_without_effect_and_shading():
    case = BY_NAME["u16_64x96_shaded"]
    img = case["image"][None]
    base = filtering.destripe_streaks_planes(img, (8.0, 8.0), out_dtype=np.float32)
    same = filtering.destripe_streaks_planes(img, (8.0, 8.0), out_dtype=np.float32, smoothing=1.0)
    assert np.array_equal(base, same)
    shaded = filtering.destripe_streaks_planes(img, (8.0, 8.0), out_dtype=np.float32, flat=case["flat"], dark=case["dark"])
    ref = soo.shade(base[0], case["flat"], case["dark"])
    assert np.all(np.abs(shaded[0] - ref) <= 1e-4 * (1 + np.abs(ref)))


def test_no_option_is_the_plain_plan():
    """smoothing=0, both bands and no flat: the bytes of a call without the arguments."""
    case = BY_NAME["u16_64x96_plain"]
    for route in ("generic", "march"):
        a = filtering.destripe_streaks_planes(case["image"][None], case["sigma"], route=route, out_dtype=np.float32)
        b = filtering.destripe_streaks_planes(case["image"][None], case["sigma"], route=route, out_dtype=np.float32,
                                              smoothing=0, flat=None, dark=None)  # fmt: skip
        assert np.array_equal(a, b)
        assert np.all(np.abs(a[0] - case["out"]) <= 1e-4 * (1 + np.abs(case["out"])))


def test_batched_equals_single_plane_calls():
    rng = np.random.default_rng(17)
    base = BY_NAME["u16_64x96_plain"]["image"]
    planes = np.stack([np.clip(base.astype(np.int64) + rng.integers(-20, 21, base.shape), 0, 65535).astype(np.uint16)
                       for _ in range(40)])  # fmt: skip
    planes[7] = 400  # a constant plane among them
    kw = dict(sigma=(None, 16.0), smoothing=1.0, out_dtype=np.float32, return_threshold=True)
    batched, tb = filtering.destripe_streaks_planes(planes, max_batch=32, **kw)
    for k in range(40):
        single, ts = filtering.destripe_streaks_planes(planes[k : k + 1], max_batch=1, **kw)
        assert np.array_equal(single[0], batched[k]), k
        assert ts[0] == tb[k]
    assert tb[7] == 400.0


# ---- through the stores -----------------------------------------------------------------------------------------------
Z, H, W = 8, 64, 96
CHUNKS = (1, 1, 4, 32, 32)
STREAKS = {"sigma": (8, 16), "smoothing": 1, "shading": True}


@pytest.fixture(scope="module")
def volume():
    rng = np.random.default_rng(23)
    base = BY_NAME["u16_64x96_plain"]["image"].astype(np.int64)
    vol = np.stack([np.clip(base + rng.integers(-30, 31, base.shape), 0, 65535).astype(np.uint16) for _ in range(Z)])
    vol.setflags(write=False)
    return vol


@pytest.fixture(scope="module")
def shading():
    case = BY_NAME["u16_64x96_smooth1_shaded"]
    return case["flat"], np.full((H + 8, W + 8), 100, np.uint16)  # the dark as the TIFF of a derivatives folder holds it


@pytest.fixture(scope="module")
def expected(volume, shading):
    out = filtering.destripe_streaks_planes(volume, (8.0, 16.0), smoothing=1.0, flat=shading[0],
                                            dark=shading[1].astype(np.float32), route="auto", out_dtype=np.uint16)  # fmt: skip
    plain = filtering.destripe_streaks_planes(volume, (8.0, 16.0), route="auto", out_dtype=np.uint16)
    assert not np.array_equal(out, plain)
    out.setflags(write=False)
    return out


def _input(tmp_path, volume, compressor):
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, Z, H, W), CHUNKS, np.uint16, compressor=compressor)
    src[0, 0] = volume
    return path


def _store(in_path, out, sc, compressor, **kw):
    n, _ = zd.destripe_zarr_store(in_path, out, None, None, sc, prediction_chunksize=(4, H, W), output_chunks=CHUNKS,
                                  device=0, compressor=compressor, io_threads=4, streaks=dict(STREAKS), **kw)  # fmt: skip
    assert n == Z
    assert zd.LAST_RUN["filter"] == "streaks"
    assert zd.LAST_RUN["streaks_smoothing"] == 1.0 and zd.LAST_RUN["streaks_shading"] is (sc is not None)
    return MiniZarrArray.open(out)[0, 0]


def test_store_voxels_are_the_filters(tmp_path, volume, shading, expected):
    sc = {"retrospective": True, "flatfield": shading[0], "darkfield": shading[1]}
    try:
        raw = _input(tmp_path, volume, None)
        assert np.array_equal(_store(raw, str(tmp_path / "raw_out"), sc, None, device_retile=True), expected)
        assert np.array_equal(_store(raw, str(tmp_path / "host_out"), sc, None, device_retile=False), expected)
        blosc = tmp_path / "blosc"
        blosc.mkdir()
        zin = _input(blosc, volume, "blosc")
        got = _store(zin, str(blosc / "out"), sc, "blosc", device_retile=True, device_codec=True)
        assert zd.LAST_RUN["device_codec"] is True
        assert np.array_equal(got, expected)
        # "shading": True without a shadow_correction runs unshaded, as the stripe filter does
        got = _store(raw, str(tmp_path / "unshaded"), None, None, device_retile=True)
        want = filtering.destripe_streaks_planes(volume, (8.0, 16.0), smoothing=1.0, route="auto", out_dtype=np.uint16)
        assert np.array_equal(got, want)
    finally:
        zd.release_staging()


def test_destripe_zarr_with_a_flatfield(tmp_path, volume, shading, expected):
    in_path = _input(tmp_path, volume, "blosc")
    d = tmp_path / "derivatives"
    d.mkdir()
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), shading[1])
    group = str(tmp_path / "destriped" / "X_0_Y_0.zarr")
    try:
        n, _ = zd.destripe_zarr(in_path, "0", group, (4, H, W), 0, 1, 1, None, str(tmp_path / "results"), str(d), None,
                                {}, device=0, output_chunks=CHUNKS, n_levels=2, io_threads=4, flatfield=shading[0],
                                streaks=dict(STREAKS))  # fmt: skip
        assert n == Z and zd.LAST_RUN["filter"] == "streaks"
        assert zd.LAST_RUN["streaks_smoothing"] == 1.0 and zd.LAST_RUN["streaks_shading"] is True
        assert np.array_equal(MiniZarrArray.open(os.path.join(group, "0"))[0, 0], expected)
    finally:
        zd.release_staging()


def test_destripe_channel_with_streaks(tmp_path, volume, shading):
    """Two tiles, one per laser side, each with the retrospective flat of its side and the dark of the derivatives
    folder: the voxels are ``destripe_streaks_planes`` of the tile with that flat."""
    chan = tmp_path / "data" / "Ex_488_Em_525"
    names = ["431040_368180", "431040_394100"]
    tiles = [volume, np.ascontiguousarray(volume[::-1])]
    flats = [shading[0], (2.0 - shading[0]).astype(np.float32)]  # both in [0.8, 1.2]
    d = tmp_path / "derivatives"
    d.mkdir()
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), shading[1])
    for name, tile, side in zip(names, tiles, (0, 1)):
        a = MiniZarrArray.create(str(chan / (name + ".zarr") / "0"), (1, 1, Z, H, W), CHUNKS, np.uint16, compressor="blosc")
        a[0, 0] = tile
        mini_tiff.imwrite(str(d / "flat_{}.tif".format(side)), flats[side])
    try:
        done = zd.destripe_channel(tmp_path / "data", d, "Ex_488_Em_525", tmp_path / "results", [1.8, 1.8, 2.0],
                                   [d / "flat_0.tif", d / "flat_1.tif"], {"0": [names[0]], "1": [names[1]]}, {},
                                   prediction_chunksize=(4, H, W), output_chunks=CHUNKS, device=0, n_levels=2,
                                   io_threads=4, streaks=dict(STREAKS))  # fmt: skip
        assert done == {names[0] + ".zarr": Z, names[1] + ".zarr": Z}
        assert zd.LAST_RUN["filter"] == "streaks" and zd.LAST_RUN["streaks_shading"] is True
        for name, tile, flat in zip(names, tiles, flats):
            want = filtering.destripe_streaks_planes(tile, (8.0, 16.0), smoothing=1.0, flat=flat,
                                                     dark=shading[1].astype(np.float32), route="auto",
                                                     out_dtype=np.uint16)  # fmt: skip
            got = MiniZarrArray.open(str(tmp_path / "results" / "destriped_data" / "Ex_488_Em_525" / (name + ".zarr") / "0"))
            assert np.array_equal(got[0, 0], want), name
    finally:
        zd.release_staging()
