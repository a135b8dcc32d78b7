"""Argument rules of the light-sheet background mode's Python layer: every ``TypeError`` / ``ValueError`` is raised
before the native library is loaded and before anything is created on disk.  No GPU needed."""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, filtering as fl, zarr_destriper as zd
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

STREAKS = {"sigma": (128, 256)}
SHADOW = {"flatfield": np.ones((8, 8), np.float32), "darkfield": np.zeros((8, 8), np.float32), "retrospective": True}

BAD_VALUES = [
    {"percentile": 0}, {"percentile": 1}, {"percentile": 1.5}, {"percentile": float("nan")}, {"percentile": "0.25"},
    {"percentile": None}, {"artifact_length": 0}, {"artifact_length": 1025}, {"artifact_length": 10.5},
    {"artifact_length": True}, {"background_window_size": 0}, {"background_window_size": 256},
    {"background_window_size": -3}, {"lightsheet_vs_background": 0}, {"lightsheet_vs_background": -2.0},
    {"lightsheet_vs_background": float("inf")}, {"lightsheet_vs_background": [2.0]},
]  # fmt: skip


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(eng_mod, "load_library", refuse)
    monkeypatch.setattr(eng_mod, "_lib", None, raising=False)


def test_options_defaults_and_values():
    assert fl.lightsheet_options({}) == dict(percentile=0.25, artifact_length=150, background_window_size=200,
                                             lightsheet_vs_background=2.0)  # fmt: skip
    opt = fl.lightsheet_options({"percentile": 0.5, "artifact_length": np.int64(1024), "background_window_size": 255.0})
    assert opt == dict(percentile=0.5, artifact_length=1024, background_window_size=255, lightsheet_vs_background=2.0)
    assert type(opt["artifact_length"]) is int and type(opt["background_window_size"]) is int
    for bad in (None, True, [("percentile", 0.25)], "lightsheet"):
        with pytest.raises(TypeError):
            fl.lightsheet_options(bad)
    for unknown in ({"sigma": 3}, {"percentile": 0.25, "rotate": True}, {1: 2}):
        with pytest.raises(TypeError):
            fl.lightsheet_options(unknown)
    for bad in BAD_VALUES:
        with pytest.raises(ValueError):
            fl.lightsheet_options(bad)
    with pytest.raises(ValueError, match="streaks"):
        fl.lightsheet_options({}, STREAKS)
    with pytest.raises(ValueError, match="shadow_correction"):
        fl.lightsheet_options({}, None, SHADOW)
    with pytest.raises(TypeError):  # the unknown key is reported whatever else is wrong
        fl.lightsheet_options({"nope": 1}, STREAKS, SHADOW)


def test_correct_lightsheet_arguments():
    plane = np.zeros((8, 8), np.uint16)
    for bad in BAD_VALUES:
        with pytest.raises(ValueError):
            fl.correct_lightsheet(plane, **bad)
        with pytest.raises(ValueError):
            fl.correct_lightsheet_planes(plane[None], **bad)
    for wrong in (plane.astype(np.float32), plane.astype(np.int16), plane.astype(np.uint8), plane.astype(np.float64)):
        with pytest.raises(ValueError, match="uint16"):
            fl.correct_lightsheet(wrong)
        with pytest.raises(ValueError, match="uint16"):
            fl.correct_lightsheet_planes(wrong[None])
    with pytest.raises(ValueError):
        fl.correct_lightsheet(plane[None])
    with pytest.raises(ValueError):
        fl.correct_lightsheet_planes(plane)
    with pytest.raises(ValueError):
        fl.correct_lightsheet_planes(np.zeros((2, 0, 8), np.uint16))
    with pytest.raises(ValueError):
        fl.correct_lightsheet_planes(plane[None], out_dtype=np.float64)
    with pytest.raises(TypeError):
        fl.correct_lightsheet(plane, rotate=1)


def _pipelines(tmp_path):
    """One call per pipeline entry point taking ``lightsheet`` and further keywords; the sources do not exist (or are
    never opened), the outputs must never appear."""
    src = tmp_path / "in"
    store = tmp_path / "in.zarr"
    MiniZarrArray.create(str(store / "0"), (1, 1, 4, 8, 8), (1, 1, 4, 8, 8), np.uint16, compressor=None)
    out = tmp_path / "out"

    def rfs(**kw):
        kw.setdefault("shadow_correction", None)
        return destriper.read_filter_save(str(out), str(src / "a.tif"), str(out / "a.tif"), None, None, **kw)

    def bf(**kw):
        return destriper.batch_filter(str(src), str(out), 1, 2, None, None, kw.pop("shadow_correction", None), **kw)

    def store_call(**kw):
        return zd.destripe_zarr_store(str(store / "0"), str(out / "0"), None, None, prediction_chunksize=(4, 8, 8),
                                      output_chunks=(1, 1, 4, 8, 8), compressor=None, **kw)  # fmt: skip

    return out, [rfs, bf, store_call]


def test_pipelines_refuse_before_anything_is_created(tmp_path):
    out, calls = _pipelines(tmp_path)
    for call in calls:
        with pytest.raises(TypeError):
            call(lightsheet={"sigma": 1})
        with pytest.raises(TypeError):
            call(lightsheet=True)
        for bad in BAD_VALUES[:3] + BAD_VALUES[6:8] + BAD_VALUES[10:12]:
            with pytest.raises(ValueError):
                call(lightsheet=bad)
        with pytest.raises(ValueError, match="streaks"):
            call(lightsheet={}, streaks=dict(STREAKS))
        with pytest.raises(ValueError, match="shadow_correction"):
            call(lightsheet={}, shadow_correction=SHADOW)
        assert not out.exists()


def test_destripe_zarr_refuses_before_anything_is_created(tmp_path):
    store = tmp_path / "t.zarr"
    MiniZarrArray.create(str(store / "0"), (1, 1, 4, 8, 8), (1, 1, 4, 8, 8), np.uint16, compressor=None)
    out = tmp_path / "res" / "t.zarr"
    deriv = tmp_path / "derivatives"

    def call(**kw):
        kw.setdefault("derivatives_path", str(tmp_path / "none"))
        kw.setdefault("flatfield", None)
        return zd.destripe_zarr(dataset_path=str(store), multiscale="0", output_destriped_zarr=str(out),
                                prediction_chunksize=(4, 8, 8), parameters={}, n_workers=1, batch_size=1,
                                super_chunksize=None, target_size_mb=1, results_folder=str(tmp_path / "results"),
                                xyz_resolution=[1.0, 1.0, 1.0], **kw)  # fmt: skip

    with pytest.raises(TypeError):
        call(lightsheet={"artifact": 3})
    with pytest.raises(ValueError):
        call(lightsheet={"percentile": 2})
    with pytest.raises(ValueError, match="streaks"):
        call(lightsheet={}, streaks=dict(STREAKS))
    with pytest.raises(ValueError, match="shadow_correction"):
        call(lightsheet={}, flatfield=np.ones((8, 8), np.float32))
    deriv.mkdir()
    with pytest.raises(ValueError, match="shadow_correction"):
        call(lightsheet={}, derivatives_path=str(deriv))
    assert not out.exists() and not (tmp_path / "res").exists()


def test_store_must_be_uint16(tmp_path):
    store = tmp_path / "f.zarr"
    MiniZarrArray.create(str(store / "0"), (1, 1, 4, 8, 8), (1, 1, 4, 8, 8), np.float32, compressor=None)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="uint16"):
        zd.destripe_zarr_store(str(store / "0"), str(out / "0"), None, None, prediction_chunksize=(4, 8, 8),
                               output_chunks=(1, 1, 4, 8, 8), compressor=None, lightsheet={})  # fmt: skip
    assert not out.exists()
