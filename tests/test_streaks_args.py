"""CPU: the ``streaks=`` option of the pipelines and the ``route=`` keyword of the dual-band filter refuse bad arguments
before any device call and before anything is created."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import destriper, engine, filtering, mini_tiff
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

STREAKS = {"sigma": (8.0, 16.0)}


def _store(tmp_path, H=64, W=96):
    path = str(tmp_path / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(path, (1, 1, 4, H, W), (1, 1, 4, 32, 32), np.uint16, compressor=None)
    src[0, 0] = np.full((4, H, W), 150, np.uint16)
    return path


def _store_kw(H=64, W=96):
    return dict(prediction_chunksize=(4, H, W), output_chunks=(1, 1, 4, 32, 32), device=0, compressor=None)


def test_streaks_with_a_shadow_correction_raises_and_creates_nothing(tmp_path):
    in_path, out = _store(tmp_path), str(tmp_path / "out" / "0")
    sc = {"retrospective": True, "flatfield": np.ones((64, 96), np.float32), "darkfield": np.zeros((64, 96), np.float32)}
    with pytest.raises(ValueError, match="dark / flat"):
        zd.destripe_zarr_store(in_path, out, None, None, sc, streaks=STREAKS, **_store_kw())
    assert not os.path.exists(str(tmp_path / "out"))

    d = tmp_path / "derivatives"
    d.mkdir()
    group = str(tmp_path / "destriped" / "X_0_Y_0.zarr")
    args = (in_path, "0", group, (4, 64, 96), 0, 1, 1, None, str(tmp_path / "results"))
    with pytest.raises(ValueError, match="dark / flat"):  # a derivatives folder that exists
        zd.destripe_zarr(*args, str(d), None, {}, streaks=STREAKS, compressor=None, output_chunks=(1, 1, 4, 32, 32))
    with pytest.raises(ValueError, match="dark / flat"):  # a retrospective flat
        zd.destripe_zarr(*args, str(tmp_path / "none"), None, {}, flatfield=sc["flatfield"], streaks=STREAKS,
                         compressor=None, output_chunks=(1, 1, 4, 32, 32))  # fmt: skip
    assert not os.path.exists(str(tmp_path / "destriped")) and not os.path.exists(str(tmp_path / "results"))

    src, dst = tmp_path / "tiffs", tmp_path / "tiffs_out"
    src.mkdir()
    dst.mkdir()
    mini_tiff.imwrite(str(src / "a.tif"), np.full((64, 96), 150, np.uint16))
    with pytest.raises(ValueError, match="dark / flat"):
        destriper.batch_filter(src, dst, 1, 4, None, None, sc, streaks=STREAKS)
    with pytest.raises(ValueError, match="dark / flat"):
        destriper.read_filter_save(dst, src / "a.tif", dst / "a.tif", None, None, sc, streaks=STREAKS)
    assert os.listdir(str(dst)) == []


def test_unknown_key_raises_type_error(tmp_path):
    in_path, out = _store(tmp_path), str(tmp_path / "out" / "0")
    bad = dict(STREAKS, sigma_fg=3.0)
    with pytest.raises(TypeError, match="sigma_fg"):
        zd.destripe_zarr_store(in_path, out, None, None, None, streaks=bad, **_store_kw())
    with pytest.raises(TypeError, match="sigma_fg"):
        destriper.batch_filter(tmp_path, tmp_path / "o", 1, 4, None, None, None, streaks=bad)
    with pytest.raises(TypeError):
        filtering.streaks_options({"level": 2})  # no sigma pair
    with pytest.raises(TypeError):
        filtering.streaks_options([("sigma", (8.0, 16.0))])
    assert not os.path.exists(str(tmp_path / "out")) and not os.path.exists(str(tmp_path / "o"))
    assert filtering.streaks_options(STREAKS) == {"sigma": (8.0, 16.0), "level": 0, "wavelet": "db3", "crossover": 10,
                                                  "threshold": -1, "route": "auto"}  # fmt: skip


def test_bad_route_raises_value_error(tmp_path):
    in_path, out = _store(tmp_path), str(tmp_path / "out" / "0")
    with pytest.raises(ValueError, match="route"):
        zd.destripe_zarr_store(in_path, out, None, None, None, streaks=dict(STREAKS, route="fast"), **_store_kw())
    odd = tmp_path / "odd"
    odd.mkdir()
    with pytest.raises(ValueError, match="march"):  # the march route on an odd plane: before the output exists
        zd.destripe_zarr_store(_store(odd, 64, 95), out, None, None, None, streaks=dict(STREAKS, route="march"),
                               **_store_kw(64, 95))  # fmt: skip
    assert not os.path.exists(str(tmp_path / "out"))
    img = np.full((64, 96), 150, np.uint16)
    with pytest.raises(ValueError, match="route"):
        filtering.filter_streaks(img, sigma=(8.0, 16.0), route="fast")
    with pytest.raises(ValueError, match="route"):
        filtering.destripe_streaks_planes(img[None], (8.0, 16.0), route=None)
    with pytest.raises(ValueError, match="march"):
        filtering.filter_streaks(img, sigma=(8.0, 16.0), wavelet="haar", route="march")
    with pytest.raises(ValueError, match="march"):
        filtering.filter_streaks(img[:, :95], sigma=(8.0, 16.0), route="march")
    assert engine.streaks_route("auto", 64, 95) == "generic" and engine.streaks_route("auto", 64, 96, "haar") == "generic"
    assert engine.streaks_route("auto", 64, 96) == engine.AUTO_ROUTE and engine.AUTO_ROUTE in ("generic", "march")
    assert engine.streaks_route("generic", 64, 96) == "generic" and engine.streaks_route("march", 64, 96) == "march"
    assert engine.streaks_route("auto", 64, 96, level=4) == "generic"  # beyond the maximum level (3)
    assert engine.streaks_route("march", 64, 96, level=3) == "march"
    with pytest.raises(ValueError, match="march"):
        engine.streaks_route("march", 64, 96, level=4)
