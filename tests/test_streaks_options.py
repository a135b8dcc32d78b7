"""CPU: the options of the dual-band filter (one-sided bands, a smoothed blend weight, dark / flat): the NumPy
restatement against the real-library fixture, the host build of the blend kernel's arithmetic against the restatement,
and the argument checks (raised before any device call)."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, engine, filtering
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.engine import streaks_blend_ref, streaks_smoothing
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from tests import streaks_options_oracle as soo

CASES = soo.golden_cases()
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def test_golden_covers_the_cases():
    assert {c["image"].shape for c in CASES} == {(64, 96), (33, 47), (20, 6)}
    assert {c["wavelet"] for c in CASES} == {"db3", "sym4", "haar"}
    assert any(c["sigma"][1] is None for c in CASES) and any(c["sigma"][0] is None for c in CASES)
    assert any(c["sigma"][1] is None and c["smoothing"] > 0 for c in CASES)
    assert any(c["flat"] is not None and c["smoothing"] > 0 for c in CASES)
    assert any(c["image"].dtype == np.float32 and c["threshold"] != -1 and c["threshold"] % 1 for c in CASES)
    for c in CASES:
        if c["flat"] is not None:  # a dark plane larger than the image, shaded values that keep 1e-4 (1 + v) < 1
            assert c["dark"].shape[0] > c["image"].shape[0] and c["dark"].shape[1] > c["image"].shape[1]
            assert 0.8 <= c["flat"].min() and c["flat"].max() <= 1.2 and c["out"].max() < 9000
    # int(4 * 2.0 + 0.5) = 8 exceeds the 6 columns: the taps fold more than once
    assert BY_NAME["u16_20x6_haar_smooth2"]["smoothing"] == 2.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_matches_golden(case):
    t, out = soo.filter_streaks(case["image"], case["sigma"], level=case["level"], wavelet=case["wavelet"],
                                crossover=case["crossover"], threshold=case["threshold"], smoothing=case["smoothing"],
                                flat=case["flat"], dark=case["dark"])  # fmt: skip
    assert t == case["t"]
    assert out.shape == case["out"].shape
    rel = np.abs(out - case["out"]) / np.maximum(np.abs(case["out"]), 1.0)
    assert rel.max() <= 1e-10, float(rel.max())
    # what a uint16 store holds: clip + truncate; a value within 1e-9 of an integer may fall on either side
    u16 = np.clip(out, 0, 65535).astype(np.uint16)
    assert np.abs(u16.astype(np.int64) - case["out_u16"]).max() <= 1
    assert np.mean(u16 == case["out_u16"]) > 0.999


def test_smoothing_changes_the_result():
    """A kernel that ignores the option cannot pass: on the 64 x 96 plane the smoothed and the raw blend differ by more
    than the bound of the GPU tests somewhere."""
    plain, smooth = BY_NAME["u16_64x96_plain"]["out"], BY_NAME["u16_64x96_smooth1"]["out"]
    assert np.any(np.abs(smooth - plain) > 1e-3 * (1 + np.abs(plain)))
    fg, fg_smooth = BY_NAME["u16_64x96_fg"]["out"], BY_NAME["u16_64x96_fg_smooth1"]["out"]
    assert np.any(np.abs(fg_smooth - fg) > 1e-3 * (1 + np.abs(fg)))
    assert np.any(np.abs(fg - plain) > 1e-3 * (1 + np.abs(plain)))
    assert np.any(np.abs(BY_NAME["u16_64x96_bg"]["out"] - plain) > 1e-3 * (1 + np.abs(plain)))


def test_fold_and_smooth_restatement():
    # d c b a | a b c d | d c b a, continued to both sides
    assert soo.fold(np.arange(-9, 13), 4).tolist() == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3]
    w = np.random.default_rng(3).random((5, 3))
    s = soo.smooth(w, 2.0)  # radius 8 on axes of 5 and 3
    assert s.shape == w.shape and abs(s.mean() - w.mean()) < 1e-12  # folding keeps the mean: every tap lands inside
    assert np.allclose(soo.smooth(np.full((4, 7), 0.25), 1.0), 0.25, atol=1e-15)


@pytest.mark.parametrize("out_dtype", [np.float32, np.uint16], ids=["f32", "u16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_blend_matches_restatement(case, out_dtype):
    """``dsx_streaks_blend_ref``: the weight, fold, tap, blend and epilogue functions the kernel is compiled from."""
    t, x, f, b = soo.bands(case["image"], case["sigma"], case["level"], case["wavelet"], case["threshold"])
    ref = soo.blend(x, f, b, t, case["crossover"], case["smoothing"], case["flat"], case["dark"])
    mode = "fg" if b is None else "bg" if f is None else "both"
    got = streaks_blend_ref(x, f, b, t, case["crossover"], bands=mode, smoothing=case["smoothing"],
                            flatfield=case["flat"], darkfield=case["dark"], out_dtype=out_dtype)  # fmt: skip
    assert got.dtype == out_dtype and got.shape == ref.shape
    if out_dtype == np.float32:
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= 1e-4 * (1 + np.abs(ref))), float((err / (1 + np.abs(ref))).max())
    else:  # 1e-4 (1 + ref) stays below one count for these planes
        assert ref.max() < 9000
        assert np.abs(got.astype(np.int64) - np.clip(ref, 0, 65535).astype(np.int64)).max() <= 1


def test_host_blend_refuses_bad_arguments():
    x = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        streaks_blend_ref(x, x, x, 1.0, smoothing=2.5)
    with pytest.raises(ValueError):
        streaks_blend_ref(x, x, x, 1.0, bands="none")
    with pytest.raises(ValueError):
        streaks_blend_ref(x, x, None, 1.0, bands="both")
    with pytest.raises(ValueError):
        streaks_blend_ref(x, x, x, 1.0, flatfield=np.ones((4, 4), np.float32))
    with pytest.raises(ValueError, match="darkfield"):
        streaks_blend_ref(x, x, x, 1.0, flatfield=np.ones((4, 4)), darkfield=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="flatfield"):
        streaks_blend_ref(x, x, x, 1.0, flatfield=np.ones((4, 5)), darkfield=np.zeros((6, 6)))


@pytest.mark.parametrize(
    "kwargs",
    [
        {"sigma": (None, None)},
        {"sigma": (8.0, 16.0), "smoothing": -1},
        {"sigma": (8.0, 16.0), "smoothing": 2.5},
        {"sigma": (8.0, 16.0), "smoothing": float("nan")},
        {"sigma": (8.0, 16.0), "smoothing": float("inf")},
        {"sigma": (8.0, None), "smoothing": "a"},
        {"sigma": (8.0, 16.0), "flat": np.ones((16, 16), np.float32)},
        {"sigma": (8.0, 16.0), "dark": np.zeros((16, 16), np.float32)},
        {"sigma": (0.0, None)},
        {"sigma": (None, -2.0)},
    ],
)
def test_option_argument_errors(kwargs):
    img = np.zeros((16, 16), np.uint16)
    with pytest.raises(ValueError):
        filtering.filter_streaks(img, **kwargs)
    kwargs = dict(kwargs)
    with pytest.raises(ValueError):
        filtering.destripe_streaks_planes(img[None], kwargs.pop("sigma"), **kwargs)


def test_plan_level_option_errors_need_no_device():
    eng = engine.DestripeEngine.__new__(engine.DestripeEngine)  # no context: a device call would fail otherwise
    for kw in ({"smoothing": -1}, {"smoothing": 2.5}, {"smoothing": float("nan")}, {"bands": "none"},
               {"flatfield": np.ones((16, 16), np.float32)},
               {"flatfield": np.ones((16, 16), np.float32), "darkfield": np.zeros((15, 16), np.float32)}):  # fmt: skip
        with pytest.raises(ValueError):
            eng.plan_streaks(16, 16, 8.0, 16.0, **kw)
    assert streaks_smoothing(0) == 0.0 and streaks_smoothing(2) == 2.0


def test_scalar_sigma_form_does_not_take_the_options():
    img = np.zeros((16, 16), np.uint16)
    with pytest.raises(TypeError):
        filtering.filter_streaks(img, sigma=8.0, smoothing=1)
    with pytest.raises(TypeError):
        filtering.filter_streaks(img, sigma=8.0, flat=np.ones((16, 16)), dark=np.zeros((16, 16)))


def test_streaks_options_dict():
    six = {"sigma": (8.0, 16.0), "level": 0, "wavelet": "db3", "crossover": 10, "threshold": -1, "route": "auto"}
    assert filtering.streaks_options({"sigma": (8.0, 16.0)}) == six
    assert filtering.streaks_options({"sigma": (8, 16), "smoothing": 1}) == dict(six, smoothing=1.0)
    assert filtering.streaks_options({"sigma": (8, 16), "shading": True}) == dict(six, shading=True)
    assert filtering.streaks_options({"sigma": (8, None), "shading": False, "smoothing": 0}) \
        == dict(six, sigma=(8.0, None), shading=False, smoothing=0.0)  # fmt: skip
    for bad in ({"sigma": (8, 16), "smoothing": 2.5}, {"sigma": (8, 16), "smoothing": -1},
                {"sigma": (8, 16), "smoothing": float("nan")}, {"sigma": (None, None)},
                {"sigma": (8, 16), "shading": "yes"}, {"sigma": (8, 16), "shading": 1}):  # fmt: skip
        with pytest.raises(ValueError):
            filtering.streaks_options(bad)
    for unknown in ({"sigma": (8, 16), "smooth": 1}, {"sigma": (8, 16), "flat": None}, {"sigma": (8, 16), "bands": "fg"}):
        with pytest.raises(TypeError):
            filtering.streaks_options(unknown)
    flat, dark = np.ones((4, 4), np.float32), np.zeros((4, 4), np.float32)
    checked = filtering.streaks_options({"sigma": (8, 16), "smoothing": 1, "shading": True})
    kw = filtering.streaks_call_options(checked, flat, dark)
    assert kw["flat"] is flat and kw["dark"] is dark and kw["smoothing"] == 1.0 and "shading" not in kw
    assert filtering.streaks_call_options(checked, None, None) == dict(six, smoothing=1.0)  # no shadow_correction: unshaded
    assert filtering.streaks_call_options(filtering.streaks_options({"sigma": (8, 16)}), flat, dark) == six


def test_shading_key_lets_a_shadow_correction_through(tmp_path):
    sc = {"retrospective": True, "flatfield": np.ones((64, 95), np.float32), "darkfield": np.zeros((64, 95), np.float32)}
    plain, shaded = {"sigma": (8.0, 16.0)}, {"sigma": (8.0, 16.0), "shading": True}
    with pytest.raises(ValueError, match="dark / flat"):
        destriper._streaks_options(plain, sc)
    with pytest.raises(ValueError, match="dark / flat"):
        destriper._streaks_options(dict(plain, shading=False), sc)
    assert destriper._streaks_options(shaded, sc)["shading"] is True
    assert destriper._streaks_options(shaded, None)["shading"] is True
    assert filtering.streaks_shading(filtering.streaks_options(shaded), sc) is sc
    # through a pipeline: with the key the call gets past the shading check to the next one (the march route refuses
    # an odd plane), without it the shading check refuses first; nothing is created either way
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, 4, 64, 95), (1, 1, 4, 32, 32), np.uint16, compressor=None)
    src[0, 0] = np.full((4, 64, 95), 150, np.uint16)
    kw = dict(prediction_chunksize=(4, 64, 95), output_chunks=(1, 1, 4, 32, 32), device=0, compressor=None)
    out = str(tmp_path / "out" / "0")
    with pytest.raises(ValueError, match="march"):
        zd.destripe_zarr_store(path, out, None, None, sc, streaks=dict(shaded, route="march"), **kw)
    with pytest.raises(ValueError, match="dark / flat"):
        zd.destripe_zarr_store(path, out, None, None, sc, streaks=dict(plain, route="march"), **kw)
    assert not os.path.exists(str(tmp_path / "out"))


def test_destripe_channel_takes_streaks_only_with_the_shading_key(tmp_path):
    args = (str(tmp_path), str(tmp_path), "Ex_561_Em_593", str(tmp_path / "results"), None, {}, {}, {})
    with pytest.raises(ValueError, match="dark / flat"):  # every tile comes with its flat there
        zd.destripe_channel(*args, streaks={"sigma": (8.0, 16.0)})
    with pytest.raises(TypeError):
        zd.destripe_channel(*args, streaks={"sigma": (8.0, 16.0), "shading": True, "flat": None})
    assert not os.path.exists(str(tmp_path / "results"))
    assert zd.destripe_channel(*args, streaks={"sigma": (8.0, 16.0), "shading": True}) == {}  # (a channel without tiles)


def test_exported_symbols():
    assert {"dsx_plan_streaks_opts", "dsx_streaks_blend_ref"} <= set(engine.EXPORTED_SYMBOLS)
