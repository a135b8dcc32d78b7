"""``aind_smartspim_destripe_amd.flatfield_estimation`` on the CPU: ``unify_fields`` against literal NumPy, the NumPy
restatement of ``scipy.ndimage.gaussian_filter`` against ``tests/golden/flat_estimation.npz``
(``tools/make_golden_flat_estimation.py``), the estimator's steps on host stacks (ranked by the host build of the
kernel), its derived recovery bound, option and argument errors, and the mirrored signatures.  No GPU needed."""

import inspect
import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import flatfield_estimation as fe
from aind_smartspim_destripe_amd import synth
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "flat_estimation.npz"))


# ---- unify_fields ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [3, 4])
def test_unify_fields_is_the_reference(count):
    rs = np.random.RandomState(5 + count)
    flats = [1.0 + 0.1 * rs.randn(6, 7) for _ in range(count)]
    darks = [90.0 + rs.randn(6, 7) for _ in range(count)]
    bases = [rs.rand(5) for _ in range(count)]
    for mode, f_op, d_op in (("median", np.median, np.median), ("mean", np.mean, np.mean), ("mip", np.max, np.min)):
        f, d, b = fe.unify_fields(flats, darks, bases, mode)
        assert f.dtype == d.dtype == b.dtype == np.float16
        assert np.array_equal(f, f_op(np.array(flats), axis=0).astype(np.float16))
        assert np.array_equal(d, d_op(np.array(darks), axis=0).astype(np.float16))
        assert np.array_equal(b, f_op(np.array(bases), axis=0).astype(np.float16))
    f, _, _ = fe.unify_fields(flats, darks, bases)  # the default is the median
    assert np.array_equal(f, np.median(np.array(flats), axis=0).astype(np.float16))
    if count == 4:  # the mean of the middle two
        s = np.sort(np.array(flats), axis=0)
        assert np.array_equal(f, ((s[1] + s[2]) / 2).astype(np.float16))
    with pytest.raises(NotImplementedError) as err:
        fe.unify_fields(flats, darks, bases, "max")
    assert str(err.value) == "Accepted values are: ['mean', 'median', 'mip']"


# ---- the restatement of scipy.ndimage.gaussian_filter ----------------------------------------------------------------
def test_the_golden_file_holds_the_five_cases():
    assert str(GOLDEN["scipy_version"])
    shapes = [(GOLDEN["plane_{}".format(i)].shape, float(GOLDEN["sigma_{}".format(i)])) for i in range(int(GOLDEN["n_cases"]))]
    assert shapes == [((24, 40), 1.5), ((24, 40), 32.0), ((7, 9), 3.0), ((1, 5), 2.0), ((33, 1), 4.0)]


@pytest.mark.parametrize("i", range(5))
def test_gaussian_smooth_is_scipy_gaussian_filter(i):
    """Two passes of at most 257 non-negative normalised taps in float64 bound the error near 1e-13 of the largest
    value; the bound asked is 1e-12."""
    plane, sigma, ref = GOLDEN["plane_{}".format(i)], float(GOLDEN["sigma_{}".format(i)]), GOLDEN["smooth_{}".format(i)]
    got = fe.gaussian_smooth(plane, sigma)
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = np.abs(got - ref).max()
    print("case", i, "max abs error", err, "relative", err / np.abs(ref).max())
    assert err <= 1e-12 * np.abs(ref).max()


def test_gaussian_smooth_zero_is_the_identity_and_scipy_is_not_imported():
    plane = GOLDEN["plane_0"]
    out = fe.gaussian_smooth(plane, 0)
    assert np.array_equal(out, plane) and out is not plane
    src = open(fe.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src


# ---- the estimator ------------------------------------------------------------------------------------------------------
def _vignette(H, W):
    """A smooth field with minimum 0.5 (the corners) and maximum 1 (the centre)."""
    y = (np.arange(H) - (H - 1) / 2) / ((H - 1) / 2)
    x = (np.arange(W) - (W - 1) / 2) / ((W - 1) / 2)
    F = 1.0 - 0.25 * (y[:, None] ** 2 + x[None, :] ** 2)
    assert F.min() == 0.5 and F.max() <= 1.0
    return F


def test_recovery_of_a_known_flat_within_the_derived_bound():
    """Planes ``floor(F b_i)`` with 9 distinct ``b_i`` of median 2000 and no smoothing: the median plane is
    ``floor(2000 F)``, off from ``2000 F`` by less than one count, and so is its mean from ``2000 mean(F)``; with
    ``F >= F_min = 0.5`` both relative errors are below ``1 / (F_min b_med) = 1e-3``, and the quotient
    ``R / mean(R)`` lies within ``1 / (1 - 1e-3) - 1 < 2.5e-3`` of ``F / mean(F)`` (the float32 cast adds 6e-8).  A
    derived bound, not a measured tolerance."""
    H, W = 48, 64
    F = _vignette(H, W)
    b = np.array([1400, 2600, 1700, 2300, 2000, 1900, 2100, 1500, 2500], np.float64)
    assert len(set(b)) == 9 and np.median(b) == 2000
    stack = np.floor(F[None] * b[:, None, None]).astype(np.uint16)
    res = fe.estimate_fields(stack, smoothing=0)
    flat = res["flatfield"]
    assert flat.dtype == np.float32 and flat.shape == (H, W)
    assert res["darkfield"] is None
    assert res["baseline"].dtype == np.float32 and res["baseline"].shape == (9,) and not res["baseline"].any()
    assert res["valid"].dtype == np.uint16 and np.all(res["valid"] == 9)
    want = F / F.mean()
    rel = np.abs(flat - want) / want
    print("largest relative error", rel.max())
    assert rel.max() <= 2.5 / (0.5 * 2000)


def test_estimate_fields_is_its_formulas():
    rs = np.random.RandomState(9)
    stack = rs.randint(100, 3000, (7, 20, 30)).astype(np.uint16)
    res = fe.estimate_fields(stack, flat_quantile=0.5, dark_quantile=0.05, smoothing=1.5, floor=0.1)
    s = np.sort(stack, axis=0)
    S = fe.gaussian_smooth(s[(500 * 6) // 1000].astype(np.float64), 1.5)
    assert np.array_equal(res["flatfield"], np.maximum(S / S.mean(), 0.1).astype(np.float32))
    assert np.array_equal(res["darkfield"], fe.gaussian_smooth(s[(50 * 6) // 1000].astype(np.float64), 1.5).astype(np.float32))
    assert res["darkfield"].dtype == np.float32


def test_unsampled_pixels_take_the_median_of_the_rest_and_floor_clamps():
    H, W = 12, 16
    stack = np.full((5, H, W), 50, np.uint16)  # below the window: unsampled
    rs = np.random.RandomState(3)
    hit = rs.rand(H, W) < 0.6
    values = rs.randint(1000, 1200, (H, W)).astype(np.uint16)
    stack[2][hit] = values[hit]
    window = (1000, 1199)
    res = fe.estimate_fields(stack, valid_range=window, smoothing=0, floor=0.1)
    assert np.array_equal(res["valid"], hit.astype(np.uint16))
    R = np.where(hit, stack.max(axis=0), 0).astype(np.float64)
    R[~hit] = np.median(R[hit])
    assert np.array_equal(res["flatfield"], np.maximum(R / R.mean(), 0.1).astype(np.float32))
    assert np.all(res["flatfield"][~hit] == np.float32(np.median(R[hit]) / R.mean()))
    # floor clamps: one valid pixel is 100 times darker than the rest
    stack = np.full((3, H, W), 2000, np.uint16)
    stack[:, 4, 5] = 20
    res = fe.estimate_fields(stack, smoothing=0, floor=0.25)
    assert res["flatfield"][4, 5] == np.float32(0.25) and res["flatfield"].min() == np.float32(0.25)
    res = fe.estimate_fields(stack, smoothing=0, floor=0.001)
    assert res["flatfield"][4, 5] == np.float32(20 / stack[0].astype(np.float64).mean())


def test_a_window_that_empties_every_pixel_raises():
    stack = np.full((4, 6, 8), 50, np.uint16)
    with pytest.raises(ValueError, match="no pixel"):
        fe.estimate_fields(stack, valid_range=(100, 200))


# ---- option and argument errors, each before any library call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call was made")

    monkeypatch.setattr(eng_mod, "load_library", refuse)
    monkeypatch.setattr(eng_mod, "DestripeEngine", refuse)
    monkeypatch.setattr(MiniZarrArray, "_read_chunk", refuse)


BAD_OPTIONS = [dict(flat_quantile=0.5004), dict(flat_quantile=1.001), dict(flat_quantile=-0.1), dict(flat_quantile="0.5"),
               dict(flat_quantile=float("nan")), dict(dark_quantile=0.12345), dict(valid_range=(5, 4)),
               dict(valid_range=(0, 65536)), dict(valid_range=(0.0, 100.0)), dict(valid_range=7), dict(smoothing=-1),
               dict(smoothing=float("inf")), dict(smoothing=None), dict(floor=0), dict(floor=float("nan")),
               dict(device=-1), dict(device=0.5)]  # fmt: skip


@pytest.mark.parametrize("options", BAD_OPTIONS, ids=[str(o) for o in BAD_OPTIONS])
def test_bad_options_are_value_errors(no_library, options):
    stack = np.zeros((3, 4, 4), np.uint16)
    with pytest.raises(ValueError):
        fe.estimate_fields(stack, **options)
    with pytest.raises(ValueError):
        fe.shading_correction(list(stack), options)


def test_quantiles_are_per_mille():
    assert fe.quantile_milli(0.5) == 500 and fe.quantile_milli(0) == 0 and fe.quantile_milli(1) == 1000
    assert fe.quantile_milli(0.29) == 290 and fe.quantile_milli(0.001 * 7) == 7
    assert fe.quantile_milli(0.5 + 5e-10) == 500
    with pytest.raises(ValueError):
        fe.quantile_milli(0.5 + 5e-9)


def test_shading_correction_argument_errors(no_library):
    stack = list(np.zeros((3, 4, 4), np.uint16))
    with pytest.raises(TypeError, match="BaSiC"):
        fe.shading_correction(stack, {"get_darkfield": True})
    with pytest.raises(TypeError, match="BaSiC"):
        fe.shading_correction(stack, {"smoothness_flatfield": 1.0, "smoothing": 2.0})
    with pytest.raises(ValueError, match="mask"):
        fe.shading_correction(stack, {}, mask=np.ones((3, 4, 4)))
    with pytest.raises(ValueError):
        fe.shading_correction(list(np.zeros((3, 4, 4), np.float32)), {})
    with pytest.raises(ValueError):
        fe.shading_correction([np.zeros((4, 4), np.uint16)] * 513, {})
    with pytest.raises(TypeError, match="BaSiC"):
        fe.slide_flat_estimation({}, "Ex_488_Em_525", [0], {"epsilon": 0.1}, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG)
    with pytest.raises(TypeError):
        fe.estimate_fields(np.zeros((3, 4, 4), np.uint16), epsilon=0.1)
    with pytest.raises(ValueError):
        fe.estimate_fields(np.zeros((3, 4, 4), np.float32))


def _channel(tmp_path, names, Z=16, H=32, W=48, cz=8):
    chan = tmp_path / "data" / "Ex_488_Em_525"
    for name in names:  # metadata only: no chunk is written, none may be read
        MiniZarrArray.create(str(chan / (name + ".zarr") / "0"), (1, 1, Z, H, W), (1, 1, cz, 16, 16), np.uint16, compressor="zlib")
    return chan


def test_estimate_channel_flats_argument_errors(tmp_path, no_library):
    names = ["431040_368180", "431040_394100"]
    _channel(tmp_path, names)
    params = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
    sides = {"0": [names[0]], "1": [names[1]]}
    args = (tmp_path / "data", "Ex_488_Em_525", sides, params, tmp_path / "flats")

    with pytest.raises(TypeError, match="BaSiC"):
        fe.estimate_channel_flats(*args, get_darkfield=True)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError):
            fe.estimate_channel_flats(*args, **bad)
    for bad in (dict(plane_step=0), dict(plane_step=2.0), dict(blocks_per_tile=0), dict(blocks_per_tile=True)):
        with pytest.raises(ValueError):
            fe.estimate_channel_flats(*args, **bad)
    with pytest.raises(TypeError):
        fe.estimate_channel_flats(*args, rotate=1)
    with pytest.raises(ValueError, match="cells_config"):
        fe.estimate_channel_flats(args[0], args[1], sides, {"cells_config": synth.CELLS_CONFIG}, args[4])
    with pytest.raises(ValueError, match="not found in"):  # the ValueError of destripe_channel
        fe.estimate_channel_flats(args[0], args[1], {"0": [names[0]]}, params, args[4])
    with pytest.raises(ValueError, match="has no tile"):
        fe.estimate_channel_flats(args[0], args[1], {"0": names, "1": []}, params, args[4])
    assert not (tmp_path / "flats").exists()


def test_more_than_512_sampled_planes_is_refused_before_any_read(tmp_path, no_library):
    names = ["431040_368180", "431040_394100"]
    _channel(tmp_path, names, Z=4096, cz=1024)
    params = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
    with pytest.raises(ValueError, match="plane_step"):  # 2 tiles x 1 block x 512 planes on one side
        fe.estimate_channel_flats(tmp_path / "data", "Ex_488_Em_525", {"0": names}, params, tmp_path / "flats", plane_step=2)
    assert fe.sampled_planes(4096, 1024, 1, 4) == list(range(2048, 3072, 4))  # 256 per tile would have passed
    assert not (tmp_path / "flats").exists()


def test_sampled_planes():
    assert fe.sampled_planes(16, 8, 1, 4) == [8, 12]  # two chunks: the first block is the centre one
    assert fe.sampled_planes(64, 8, 1, 8) == [32]
    assert fe.sampled_planes(64, 8, 2, 4) == [16, 20, 48, 52]
    assert fe.sampled_planes(20, 8, 3, 3) == [0, 3, 6, 8, 11, 14, 16, 19]  # the last chunk is short
    assert fe.sampled_planes(5, 8, 4, 2) == [0, 2, 4]  # more blocks than chunks: each chunk once


# ---- signatures -----------------------------------------------------------------------------------------------------------
def test_the_mirrored_functions_take_the_reference_parameters():
    """Names and order of ``flatfield_estimation.py`` of the reference, as literal lists."""
    want = {
        "shading_correction": ["slides", "shading_parameters", "mask"],
        "unify_fields": ["flatfields", "darkfields", "baselines", "mode"],
        "slide_flat_estimation": ["dict_struct", "channel_name", "slide_idxs", "shading_parameters", "no_cells_config",
                                  "cells_config"],  # fmt: skip
    }
    for name, params in want.items():
        sig = inspect.signature(getattr(fe, name))
        assert list(sig.parameters) == params, name
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert inspect.signature(fe.shading_correction).parameters["mask"].default is None
    assert inspect.signature(fe.unify_fields).parameters["mode"].default == "median"
    sig = inspect.signature(fe.estimate_channel_flats)
    assert list(sig.parameters)[:5] == ["zarr_dataset_path", "channel_name", "laser_tiles", "parameters", "output_folder"]
    for name in ("multiscale", "blocks_per_tile", "plane_step", "microscope_high_int", "rotate", "device"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert (sig.parameters["multiscale"].default, sig.parameters["blocks_per_tile"].default,
            sig.parameters["plane_step"].default, sig.parameters["microscope_high_int"].default) == ("0", 1, 8, 2700)  # fmt: skip
    sig = inspect.signature(fe.estimate_fields)
    assert [p for p in sig.parameters][1:] == list(fe.ESTIMATOR_OPTIONS)
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[1:])
