"""``flatfield_estimation`` on the device: ``estimate_channel_flats`` over a small channel of two laser sides against the
same estimator run on the host over ``filtering.destripe_planes`` of the same sampled planes, bit for bit (the rank step
is integer-exact and the rest is the same host code); the record, the hand-over to ``destripe_channel``,
``slide_flat_estimation`` on a TIFF tree, ``shading_correction``, and a plane of odd size."""

import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import filtering, mini_tiff, synth
from aind_smartspim_destripe_amd import flatfield_estimation as fe
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

CHANNEL = "Ex_488_Em_525"
PARAMS = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
NAMES = ["431040_368180", "431040_394100", "457080_368180", "457080_394100"]
SIDES = {"0": NAMES[:2], "1": NAMES[2:]}
OPTIONS = dict(smoothing=2.0, dark_quantile=0.05)


def _vignette(H, W):
    y = (np.arange(H) - (H - 1) / 2) / ((H - 1) / 2)
    x = (np.arange(W) - (W - 1) / 2) / ((W - 1) / 2)
    return 1.0 - 0.25 * (y[:, None] ** 2 + x[None, :] ** 2)


def _volume(t, Z, H, W):
    vol = synth.synthetic_stack(Z, H, W, n_unique=8).astype(np.float64) * (4.0 + t) * _vignette(H, W)[None]
    return np.clip(vol, 0, 65535).astype(np.uint16)


def _channel(root, sides, Z=16, H=32, W=48):
    vols = {}
    for names in sides.values():
        for name in names:
            a = MiniZarrArray.create(str(root / "data" / CHANNEL / (name + ".zarr") / "0"), (1, 1, Z, H, W), (1, 1, 8, 16, 16),
                                     np.uint16, compressor="zlib")  # fmt: skip
            vols[name] = _volume(NAMES.index(name), Z, H, W)
            a[0, 0] = vols[name]
    return vols


def _host_flat(vols, names, zs, **options):
    """The estimator on the host: the sampled planes of every tile through ``filtering.destripe_planes`` (unshaded,
    uint16), stacked, cropped to the tile's shape, and ``estimate_fields`` with the host build of the rank step."""
    H, W = vols[names[0]].shape[1:]
    tiles = [filtering.destripe_planes(vols[name][zs], name, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, 2700,
                                       out_dtype=np.uint16) for name in names]  # fmt: skip
    stack = np.ascontiguousarray(np.concatenate(tiles)[:, :H, :W])
    return fe.estimate_fields(stack, **options), stack


@pytest.fixture(scope="module")
def channel(tmp_path_factory):
    root = tmp_path_factory.mktemp("flat_channel")
    vols = _channel(root, SIDES)
    paths = fe.estimate_channel_flats(root / "data", CHANNEL, SIDES, PARAMS, root / "flats", plane_step=4, **OPTIONS)
    return root, vols, paths, dict(fe.LAST_ESTIMATE)


def test_the_written_flats_equal_the_host_estimator_bit_for_bit(channel):
    root, vols, paths, _ = channel
    assert [os.path.basename(p) for p in paths] == ["estimated_flat_laser_{}_{}.tif".format(CHANNEL, s) for s in ("0", "1")]
    zs = fe.sampled_planes(16, 8, 1, 4)
    assert zs == [8, 12]
    flats = []
    for path, side in zip(paths, ("0", "1")):
        got = mini_tiff.imread(path)
        want, stack = _host_flat(vols, SIDES[side], zs, **OPTIONS)
        assert stack.shape == (4, 32, 48)
        assert got.dtype == np.float32 and got.shape == (32, 48)
        assert got.tobytes() == want["flatfield"].tobytes()
        flats.append(got)
    assert not np.array_equal(flats[0], flats[1])  # the sides hold different tiles
    centre, corner = flats[0][12:20, 18:30].mean(), flats[0][:4, :4].mean()
    assert corner < centre  # the vignette is in the flat


def test_the_record_says_what_ran(channel):
    _, _, paths, last = channel
    assert last["planes"] == {"0": 4, "1": 4}
    assert last["valid_range"] == (0, 65535)
    assert last["quantiles"] == {"flat": 0.5, "dark": 0.05}
    assert sorted(last["seconds"]) == ["destripe", "estimate", "read", "write"]
    assert all(v >= 0 for v in last["seconds"].values())
    assert last["paths"] == paths


def test_the_paths_run_destripe_channel(channel):
    root, vols, paths, _ = channel
    d = root / "derivatives"
    d.mkdir(exist_ok=True)
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), np.full((40, 56), 90, np.uint16))
    done = zd.destripe_channel(zarr_dataset_path=root / "data", derivatives_path=d, channel_name=CHANNEL,
                               results_folder=root / "results", xyz_resolution=[1.8, 1.8, 2.0],
                               estimated_channel_flats=paths, laser_tiles=SIDES, parameters=PARAMS,
                               prediction_chunksize=(8, 32, 48), output_chunks=(1, 1, 8, 16, 16), compressor="zlib",
                               device=0)  # fmt: skip
    assert done == {name + ".zarr": 16 for name in NAMES}
    out = MiniZarrArray.open(str(root / "results" / "destriped_data" / CHANNEL / (NAMES[0] + ".zarr") / "0"))
    assert out.shape == (1, 1, 16, 32, 48) and out[0, 0].any()


def test_an_odd_plane_gives_a_flat_of_its_own_shape(tmp_path):
    sides = {"0": [NAMES[0]]}
    vols = _channel(tmp_path, sides, Z=8, H=31, W=47)
    (path,) = fe.estimate_channel_flats(tmp_path / "data", CHANNEL, sides, PARAMS, tmp_path / "flats", plane_step=2,
                                        smoothing=1.0)  # fmt: skip
    got = mini_tiff.imread(path)
    assert got.shape == (31, 47) and got.dtype == np.float32
    assert fe.LAST_ESTIMATE["planes"] == {"0": 4}
    want, stack = _host_flat(vols, sides["0"], fe.sampled_planes(8, 8, 1, 2), smoothing=1.0)
    assert stack.shape == (4, 31, 47)
    assert got.tobytes() == want["flatfield"].tobytes()


def test_slide_flat_estimation_on_a_tiff_tree(tmp_path, monkeypatch):
    cols, rows, slides = ["431040", "457080"], ["368180", "394100"], ["000000.tif", "000020.tif"]
    k = 0
    struct = {CHANNEL: {}}
    for col in cols:
        struct[CHANNEL][col] = {}
        for row in rows:
            folder = tmp_path / CHANNEL / col / "{}_{}".format(col, row)
            folder.mkdir(parents=True)
            struct[CHANNEL][col]["{}_{}".format(col, row)] = list(slides)
            for slide in slides:
                plane = np.clip(synth.synthetic_plane(k, 32, 48) * 5.0 * _vignette(32, 48), 0, 65535).astype(np.uint16)
                mini_tiff.imwrite(str(folder / slide), plane)
                k += 1
    monkeypatch.chdir(tmp_path)  # the reference builds its tile paths relative to the channel name
    options = {"smoothing": 1.5, "dark_quantile": 0.25}
    res = fe.slide_flat_estimation(struct, CHANNEL, [0, 1], options, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG)
    assert sorted(res) == [0, 1]
    for idx in (0, 1):
        r = res[idx]
        assert sorted(r) == ["baseline", "darkfield", "data", "flatfield"]
        assert len(r["data"]) == 4 and all(t.shape == (32, 48) and t.dtype == np.uint16 for t in r["data"])
        raw = np.stack([mini_tiff.imread(str(tmp_path / CHANNEL / c / "{}_{}".format(c, w) / slides[idx])) for c in cols for w in rows])
        want_data = filtering.destripe_planes(raw, "tile", synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, 2700, out_dtype=np.uint16)
        assert np.array_equal(np.stack(r["data"]), want_data)
        want = fe.estimate_fields(np.stack(r["data"]), **options)
        assert r["flatfield"].tobytes() == want["flatfield"].tobytes()
        assert r["darkfield"].tobytes() == want["darkfield"].tobytes()
        assert r["baseline"].shape == (4,) and not r["baseline"].any()
    # shading_correction over the downloaded tiles: the same fields through the device once more
    again = fe.shading_correction(res[0]["data"], options)
    assert sorted(again) == ["baseline", "darkfield", "flatfield"]
    assert again["flatfield"].tobytes() == res[0]["flatfield"].tobytes()
    assert again["darkfield"].tobytes() == res[0]["darkfield"].tobytes()
