"""CPU: the NumPy restatement of the dual-band filter against the real-library fixtures, and the argument checks of
the dual-band ``filter_streaks`` / ``destripe_streaks_planes`` (raised before any device call)."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import filtering
from tests import streaks_oracle as so

GOLDEN = [os.path.join(os.path.dirname(__file__), "golden", f) for f in ("streaks.npz", "streaks_256.npz")]
CASES = list(so.golden_cases(GOLDEN))


def test_golden_covers_the_cases():
    names = {c["name"] for c in CASES}
    assert {"db3_64_u16", "db3_96x130_f32", "db3_127x201_u16_odd", "db3_256_u16"} <= names
    odd_one_axis = [c for c in CASES if (c["image"].shape[0] % 2) != (c["image"].shape[1] % 2)]
    assert any(c["sigma"][0] != c["sigma"][1] for c in odd_one_axis)
    assert {c["wavelet"] for c in CASES} >= {"db3", "haar", "sym4"}
    assert {c["image"].dtype for c in CASES} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert any(c["sigma"][0] == c["sigma"][1] for c in CASES)
    assert any(c["threshold"] != -1 for c in CASES)
    assert any(c["level"] > 0 for c in CASES) and any(c["level"] == 0 for c in CASES)
    assert len({c["crossover"] for c in CASES}) >= 2


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_golden(case):
    t, out = so.filter_streaks(case["image"], case["sigma"], level=case["level"], wavelet=case["wavelet"],
                               crossover=case["crossover"], threshold=case["threshold"])  # fmt: skip
    assert t == case["t"]
    assert out.shape == case["out"].shape
    rel = np.abs(out - case["out"]) / np.maximum(np.abs(case["out"]), 1.0)
    assert rel.max() <= 1e-11, float(rel.max())


@pytest.mark.parametrize("case", [c for c in CASES if c["threshold"] == -1], ids=lambda c: c["name"])
def test_otsu_bin_and_no_plateau(case):
    t, k = so.threshold_otsu(case["image"])
    assert t == case["t"]
    assert k == case["otsu_bin"]
    if case["image"].dtype == np.float32 and case["image"].min() != case["image"].max():
        counts, edges = so.orc.histogram256(case["image"])
        _, var = so.orc.otsu_variance_curve(counts, edges)
        # the maximum is one contiguous run starting at k (empty bins repeat a value exactly) and clear of every other
        # value of the curve, so float32 rounding on the device cannot move the first maximum to another bin
        run = int(np.sum(var == var[k]))
        assert np.all(var[k : k + run] == var[k])
        assert var[var != var[k]].max() < var[k] * (1 - 1e-6)


def test_integer_otsu_of_a_poisson_plane():
    img = np.random.default_rng(0).poisson(200, size=(64, 64)).astype(np.uint16)
    t, k = so.threshold_otsu(img)
    assert float(t) == float(int(t)) and k == int(t) - int(img.min())


@pytest.mark.parametrize(
    "kwargs",
    [
        {"sigma": [8.0]},
        {"sigma": [8.0, 16.0, 32.0]},
        {"sigma": (0.0, 16.0)},
        {"sigma": (8.0, -1.0)},
        {"sigma": (8.0, 16.0), "crossover": 0},
        {"sigma": (8.0, 16.0), "crossover": -5},
        {"sigma": (8.0, 16.0), "wavelet": "dmey"},
        {"sigma": (8.0, 16.0), "wavelet": "nope"},
        {"sigma": (8.0, 16.0), "level": -1},
        {"sigma": np.array([[8.0, 16.0]])},
    ],
)
def test_dual_band_argument_errors(kwargs):
    img = np.zeros((16, 16), np.uint16)
    with pytest.raises(ValueError):
        filtering.filter_streaks(img, **kwargs)
    with pytest.raises(ValueError):
        filtering.destripe_streaks_planes(img[None], kwargs.pop("sigma"), **kwargs)


def test_scalar_sigma_form_does_not_take_crossover():
    with pytest.raises(TypeError):
        filtering.filter_streaks(np.zeros((16, 16), np.uint16), sigma=8.0, crossover=20)
