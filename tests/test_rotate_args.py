"""``rotate`` at the public interface, on the CPU: anything but a bool raises ``TypeError`` before the library or a
device is touched, the ``streaks=`` dict takes the key ``"rotate"`` (and still refuses unknown keys), and the
scalar-``sigma`` form of ``filter_streaks`` hands the option on."""

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, engine, synth
from aind_smartspim_destripe_amd import filtering as fl
from aind_smartspim_destripe_amd import zarr_destriper as zd

BAD = [1, 0, "yes", None, 1.0]
_ENGINE_CLASS = engine.DestripeEngine  # (the fixture below replaces the module attribute)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("library call {} before the argument check".format(name))


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library or of an engine fails the test."""

    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")

    monkeypatch.setattr(engine, "load_library", boom)
    monkeypatch.setattr(engine, "DestripeEngine", boom)
    monkeypatch.setattr(engine, "_lib", None)


def _bare_engine():
    e = object.__new__(_ENGINE_CLASS)
    e._lib, e._ctx = _NoLibrary(), None
    return e


PLANE = np.ones((8, 12), np.uint16)
CFG = synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG


def _calls(tmp_path):
    e = _bare_engine()
    zarr14 = dict(dataset_path=tmp_path / "a.zarr", multiscale="0", output_destriped_zarr=tmp_path / "o.zarr",
                  prediction_chunksize=(4, 8, 12), target_size_mb=1, n_workers=0, batch_size=1, super_chunksize=(4, 8, 12),
                  results_folder=tmp_path, derivatives_path=tmp_path, xyz_resolution=[1, 1, 1],
                  parameters={"cells_config": CFG[0], "no_cells_config": CFG[1]})  # fmt: skip
    return {
        "DestripeEngine.plan": lambda r: e.plan(8, 12, *CFG, rotate=r),
        "DestripeEngine.plan_streaks": lambda r: e.plan_streaks(8, 12, 64, 128, rotate=r),
        "get_engine": lambda r: fl.get_engine((8, 12), *CFG, rotate=r),
        "_streaks_engine": lambda r: fl._streaks_engine((8, 12), 64.0, 128.0, 0, "db3", 10, -1, 1, 0, rotate=r),
        "log_space_fft_filtering": lambda r: fl.log_space_fft_filtering(PLANE, rotate=r),
        "filter_stripes": lambda r: fl.filter_stripes(PLANE, "X_0_Y_0", CFG[1], CFG[0], rotate=r),
        "destripe_planes": lambda r: fl.destripe_planes(PLANE[None], "X_0_Y_0", CFG[1], CFG[0], rotate=r),
        "destripe_planes (two wavelets)": lambda r: fl.destripe_planes(
            PLANE[None], "X_0_Y_0", dict(CFG[1], wavelet="db2"), CFG[0], rotate=r),
        "filter_streaks (scalar)": lambda r: fl.filter_streaks(PLANE, sigma=64, rotate=r),
        "filter_streaks (pair)": lambda r: fl.filter_streaks(PLANE, sigma=(64, 128), rotate=r),
        "destripe_streaks_planes": lambda r: fl.destripe_streaks_planes(PLANE[None], (64, 128), rotate=r),
        "streaks_options": lambda r: fl.streaks_options({"sigma": (64, 128), "rotate": r}),
        "execute_worker": lambda r: zd.execute_worker(PLANE[None, None], None, None, CFG[0], CFG[1], (0, 0, 0), None, None,
                                                      "t.zarr", None, rotate=r),  # fmt: skip
        "destripe_zarr_store": lambda r: zd.destripe_zarr_store(tmp_path / "a", tmp_path / "o", *CFG, rotate=r),
        "destripe_zarr_store (dict)": lambda r: zd.destripe_zarr_store(
            tmp_path / "a", tmp_path / "o", None, None, streaks={"sigma": (64, 128), "rotate": r}),
        "destripe_zarr": lambda r: zd.destripe_zarr(**zarr14, rotate=r),
        "destripe_channel": lambda r: zd.destripe_channel(tmp_path, tmp_path, "Ex_488_Em_525", tmp_path, [1, 1, 1], [], {},
                                                          zarr14["parameters"], rotate=r),  # fmt: skip
        "read_filter_save": lambda r: destriper.read_filter_save(tmp_path, tmp_path / "a.tif", tmp_path / "b.tif", CFG[0],
                                                                 CFG[1], rotate=r),  # fmt: skip
        "batch_filter": lambda r: destriper.batch_filter(tmp_path / "in", tmp_path / "out", 1, 1, CFG[0], CFG[1], None,
                                                         rotate=r),  # fmt: skip
        "batch_filter (dict)": lambda r: destriper.batch_filter(tmp_path / "in", tmp_path / "out", 1, 1, CFG[0], CFG[1],
                                                                None, streaks={"sigma": (64, 128), "rotate": r}),  # fmt: skip
    }


def test_a_rotate_that_is_no_bool_is_a_type_error_before_any_library_call(tmp_path, no_device):
    calls = _calls(tmp_path)
    for name, call in calls.items():
        for bad in BAD:
            with pytest.raises(TypeError, match="rotate"):
                call(bad)
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists() and not (tmp_path / "o.zarr").exists()


def test_streaks_dict_takes_rotate_and_still_refuses_unknown_keys():
    opt = fl.streaks_options({"sigma": (64, 128), "rotate": True})
    assert opt["rotate"] is True
    assert "rotate" not in fl.streaks_options({"sigma": (64, 128)})
    assert fl.streaks_options({"sigma": (64, 128), "rotate": np.bool_(False)})["rotate"] is False
    with pytest.raises(TypeError, match="unexpected keys"):
        fl.streaks_options({"sigma": (64, 128), "rotate": True, "rotation": 90})
    with pytest.raises(TypeError, match="unexpected keys"):
        fl.streaks_options({"sigma": (64, 128), "angle": 90})
    kw = fl.streaks_call_options(opt)
    assert kw["rotate"] is True and "shading" not in kw


def test_scalar_sigma_form_of_filter_streaks_forwards_rotate(monkeypatch):
    seen = {}

    def fake(input_image, wavelet="db3", level=0, sigma=64, max_threshold=4, *, rotate=False):
        seen.update(sigma=sigma, rotate=rotate, max_threshold=max_threshold)
        return "filtered"

    monkeypatch.setattr(fl, "log_space_fft_filtering", fake)
    assert fl.filter_streaks(PLANE, sigma=32, rotate=True, max_threshold=3) == "filtered"
    assert seen == {"sigma": 32, "rotate": True, "max_threshold": 3}
    fl.filter_streaks(PLANE, sigma=32)
    assert seen["rotate"] is False


def test_engine_caches_are_keyed_on_rotate(monkeypatch):
    """Two plans that differ in nothing but ``rotate`` are two engines."""
    made = []

    class FakeEngine:
        def __init__(self, device):
            made.append(self)

        def plan(self, *a, rotate=False, **k):
            self.rotate = rotate

        def plan_streaks(self, *a, rotate=False, **k):
            self.rotate = rotate

        def close(self):
            pass

    monkeypatch.setattr(engine, "DestripeEngine", FakeEngine)
    monkeypatch.setattr(fl, "_ENGINES", type(fl._ENGINES)())
    a = fl.get_engine((8, 12), *CFG)
    b = fl.get_engine((8, 12), *CFG, rotate=True)
    assert a is not b and (a.rotate, b.rotate) == (False, True)
    assert fl.get_engine((8, 12), *CFG, rotate=True) is b and fl.get_engine((8, 12), *CFG) is a
    c = fl._streaks_engine((8, 12), 64.0, 128.0, 0, "db3", 10, -1, 1, 0)
    d = fl._streaks_engine((8, 12), 64.0, 128.0, 0, "db3", 10, -1, 1, 0, rotate=True)
    assert c is not d and (c.rotate, d.rotate) == (False, True) and len(made) == 4
