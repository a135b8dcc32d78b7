"""The OME-NGFF metadata of a multiscale group (``zarr_destriper.write_ome_ngff_metadata`` and its helpers, restated
from the reference's ``zarr_destriper.py:410-674``), the display window from a histogram against ``np.percentile``, the
option rules of the entry points, and ``RankGroup.sum_counts``.  No GPU needed."""

import json
import os
import sys

import numpy as np
import pytest

from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AXES = [
    {"name": "t", "type": "time", "unit": "millisecond"},
    {"name": "c", "type": "channel"},
    {"name": "z", "type": "space", "unit": "micrometer"},
    {"name": "y", "type": "space", "unit": "micrometer"},
    {"name": "x", "type": "space", "unit": "micrometer"},
]

# derived by hand from the reference's source (zarr_destriper.py:410-674, 713-741) for the input of _Arr below
EXPECTED = {
    "omero": {
        "id": 1,
        "name": "t.zarr",
        "version": "0.4",
        "channels": [
            {
                "active": True,
                "coefficient": 1,
                "color": "690afe",
                "family": "linear",
                "inverted": False,
                "label": "t.zarr",
                "window": {"end": 350.0, "max": 65535.0, "min": 0.0, "start": 0.0},
            }
        ],
        "rdefs": {"defaultT": 0, "defaultZ": 4, "model": "color"},
    },
    "multiscales": [
        {
            "version": "0.4",
            "name": "/",
            "axes": AXES,
            "datasets": [
                {"path": "0", "coordinateTransformations": [{"type": "scale", "scale": [1.0, 1.0, 2.0, 1.8, 1.8]}]},
                {"path": "1", "coordinateTransformations": [{"type": "scale", "scale": [1.0, 1.0, 4.0, 3.6, 3.6]}]},
                {"path": "2", "coordinateTransformations": [{"type": "scale", "scale": [1.0, 1.0, 8.0, 7.2, 7.2]}]},
            ],
        }
    ],
}


class _Arr:
    shape = (1, 1, 8, 32, 48)
    chunks = (1, 1, 4, 16, 16)


class _DaskLike:
    shape = (1, 1, 8, 32, 48)
    chunksize = (1, 1, 4, 16, 16)


class _Group:
    def __init__(self, path):
        self.path = path


def _write(group, arr=_Arr, **kw):
    zd.write_ome_ngff_metadata(group, arr, "t.zarr", 3, [2, 2, 2], [2.0, 1.8, 1.8], channel_names=["t.zarr"],
                               channel_colors=[0x690AFE], channel_minmax=[(0, 65535)],
                               channel_startend=[(0.0, 350.0)], **kw)  # fmt: skip


def _attrs(group):
    with open(os.path.join(str(group), ".zattrs")) as f:
        return json.load(f)


def test_zattrs_are_the_reference_values(tmp_path):
    g = tmp_path / "g.zarr"
    _write(str(g))
    assert _attrs(g) == EXPECTED
    with open(os.path.join(str(g), ".zgroup")) as f:
        assert json.load(f) == {"zarr_format": 2}
    assert sorted(os.listdir(str(g))) == [".zattrs", ".zgroup"]  # no temporary file is left
    h = tmp_path / "h.zarr"
    _write(_Group(str(h)), arr=_DaskLike)  # anything with .path / .chunksize
    assert _attrs(h) == EXPECTED


def test_float_products_are_the_references():
    """Level scales are running products (last scale times the factor), as the reference computes them."""
    t, _ = zd._compute_scales(4, [2, 2, 2], [2.0, 1.8, 1.8], (1, 1, 4, 16, 16), (1, 1, 8, 32, 48))
    s = [2.0, 1.8, 1.8]
    for level in range(4):
        assert t[level] == [{"type": "scale", "scale": [1.0, 1.0] + s}]
        s = [v * 2 for v in s]


def test_compute_scales_chunk_options_clamp_to_the_level_shapes():
    _, opts = zd._compute_scales(4, (2, 2, 2), (1.0, 1.0, 1.0), (1, 1, 4, 16, 16), (1, 1, 9, 33, 20))
    assert opts == [{"chunks": (1, 1, 4, 16, 16)}, {"chunks": (1, 1, 4, 16, 10)}, {"chunks": (1, 1, 3, 9, 5)},
                    {"chunks": (1, 1, 2, 5, 3)}]  # fmt: skip  (shapes 9x33x20, 5x17x10, 3x9x5, 2x5x3: halves round up)
    t, opts = zd._compute_scales(1, (2, 2, 2), (1.0, 2.0, 3.0), (1, 1, 64, 128, 128), (1, 1, 8, 32, 48))
    assert len(t) == 1 and opts == [{"chunks": (1, 1, 8, 32, 48)}]


def test_translation_is_appended_to_every_level():
    tr = [0.0, 0.0, 10.0, 20.0, 30.0]
    t, _ = zd._compute_scales(3, (2, 2, 2), (2.0, 1.8, 1.8), (1, 1, 4, 16, 16), (1, 1, 8, 32, 48), translation=tr)
    assert len(t) == 3
    for level in t:
        assert [e["type"] for e in level] == ["scale", "translation"] and level[1]["translation"] == tr
    zd._validate_coordinate_transformations(5, 3, t)


def test_build_ome_defaults():
    ome = zd._build_ome((1, 2, 9, 4, 4), "img")
    assert [c["label"] for c in ome["channels"]] == ["Channel:img:0", "Channel:img:1"]
    assert [c["color"] for c in ome["channels"]] == ["000000", "000001"]
    assert ome["channels"][1]["window"] == {"end": 1.0, "max": 1.0, "min": 0.0, "start": 0.0}
    assert ome["rdefs"]["defaultZ"] == 4
    assert zd._get_axes_5d() == AXES
    assert zd._get_axes_5d("second", "nanometer")[0]["unit"] == "second"


def test_extra_metadata_lands_in_the_multiscales_entry(tmp_path):
    g = str(tmp_path / "g.zarr")
    _write(g, metadata={"type": "mean", "metadata": {"method": "windowed_mean"}})
    entry = _attrs(g)["multiscales"][0]
    assert entry["type"] == "mean" and entry["metadata"] == {"method": "windowed_mean"}
    assert {k: v for k, v in entry.items() if k not in ("type", "metadata")} == EXPECTED["multiscales"][0]


def test_foreign_keys_of_an_existing_zattrs_survive(tmp_path):
    g = str(tmp_path / "g.zarr")
    os.makedirs(g)
    with open(os.path.join(g, ".zattrs"), "w") as f:
        json.dump({"acquisition": {"id": 7}, "omero": {"stale": True}}, f)
    _write(g)
    got = _attrs(g)
    assert got.pop("acquisition") == {"id": 7}
    assert got == EXPECTED


def test_coordinate_transformation_checks():
    scale = {"type": "scale", "scale": [1.0] * 5}
    tr = {"type": "translation", "translation": [0.0] * 5}
    zd._validate_coordinate_transformations(5, 2, [[scale], [scale, tr]])
    bad = [
        [[scale]],  # one list per level
        [[scale], [tr, scale]],  # the scale comes first
        [[scale], [scale, scale]],  # exactly one scale
        [[scale], [tr]],
        [[scale], [scale, tr, tr]],  # at most one translation
        [[scale], [{"type": "scale", "scale": [1.0] * 4}]],  # of length 5
        [[scale], [scale, {"type": "translation", "translation": [0.0] * 3}]],
        [[scale], [{"type": "scale", "scale": [1.0, 1.0, "a", 1.0, 1.0]}]],
        [[scale], [scale, {"type": "rotation", "rotation": [0.0] * 5}]],
    ]
    for t in bad:
        with pytest.raises(ValueError):
            zd._validate_coordinate_transformations(5, 2, t)


def test_write_refuses_before_a_file_exists(tmp_path):
    g = str(tmp_path / "g.zarr")
    with pytest.raises(ValueError):  # three voxel sizes make a scale of length 5; two do not
        zd.write_ome_ngff_metadata(g, _Arr, "t", 3, [2, 2, 2], [2.0, 1.8])
    with pytest.raises(ValueError):
        zd.write_ome_ngff_metadata(g, _Arr, "t", 3, [2, 2, 2], [2.0, "a", 1.8])

    class Flat:
        shape, chunks = (8, 32, 48), (4, 16, 16)

    with pytest.raises(ValueError):
        zd.write_ome_ngff_metadata(g, Flat, "t", 3, [2, 2, 2], [2.0, 1.8, 1.8])
    assert not os.path.exists(g)


# ---- the display window ---------------------------------------------------------------------------------------------
QS = (0, 0.1, 50, 95, 100)


def _window_ref(v, qs):
    lo, hi = (float(np.percentile(v, q, method="lower")) for q in qs)
    return lo, max(hi, lo + 1.0)


def test_display_window_is_numpys_lower_percentile():
    rs = np.random.RandomState(5)
    for case in range(200):
        n = int(rs.randint(1, 3000))
        top = int(rs.choice([2, 7, 300, 65536]))
        v = rs.randint(0, top, n).astype(np.uint16)
        hist = np.bincount(v, minlength=65536)
        for q0 in QS:
            for q1 in QS:
                assert zd.display_window_from_histogram(hist, (q0, q1)) == _window_ref(v, (q0, q1)), (case, n, q0, q1)
        got = zd.display_window_from_histogram(hist)
        assert got == _window_ref(v, (0.1, 95.0)) and all(isinstance(x, float) for x in got)


def test_display_window_of_constant_and_two_valued_volumes():
    const = np.full(1000, 150, np.uint16)
    assert zd.display_window_from_histogram(np.bincount(const, minlength=65536)) == (150.0, 151.0)
    top = np.full(10, 65535, np.uint16)
    assert zd.display_window_from_histogram(np.bincount(top, minlength=65536)) == (65535.0, 65536.0)
    for n_hi in (1, 50, 51, 999):
        two = np.concatenate([np.full(1000 - n_hi, 100, np.uint16), np.full(n_hi, 4000, np.uint16)])
        hist = np.bincount(two, minlength=65536)
        for q0 in QS:
            for q1 in QS:
                assert zd.display_window_from_histogram(hist, (q0, q1)) == _window_ref(two, (q0, q1)), (n_hi, q0, q1)


def test_display_window_refuses_an_empty_histogram():
    with pytest.raises(ValueError):
        zd.display_window_from_histogram(np.zeros(65536, np.int64))
    with pytest.raises(ValueError):
        zd.display_window_from_histogram(np.ones(65536, np.int64), (0.1, 101.0))
    with pytest.raises(ValueError):
        zd.display_window_from_histogram(np.ones(65536, np.float64))


# ---- the options of the entry points: every error before a file exists --------------------------------------------
def _level0(tmp_path):
    """A finished level 0 (host writer) for compute_multiscale; its errors must come before a level or a file."""
    g = str(tmp_path / "g.zarr")
    arr = MiniZarrArray.create(os.path.join(g, "0"), (1, 1, 8, 32, 48), (1, 1, 4, 16, 16), np.uint16, compressor=None)
    arr[0, 0] = np.arange(8 * 32 * 48, dtype=np.uint16).reshape(8, 32, 48)
    return g


def _multiscale(g, voxel_size=(2.0, 1.8, 1.8), image_name="t.zarr", **kw):
    return zd.compute_multiscale(os.path.join(g, "0"), g, [2, 2, 2], 1, voxel_size, image_name, n_levels=3,
                                 chunks=(1, 1, 4, 16, 16), compressor=None, **kw)  # fmt: skip


@pytest.mark.parametrize("kw", [
    dict(display_window=(0.0, 10.0)),  # display_window without ome_metadata
    dict(histogram=np.ones(65536, np.int64)),  # histogram without ome_metadata
    dict(display_window="percentile", histogram=np.ones(65536, np.int64)),
    dict(ome_metadata=True, display_window="percentile"),  # needs the histogram
    dict(ome_metadata=True, display_window="percentile", histogram=np.zeros(65536, np.int64)),  # an empty one
    dict(ome_metadata=True, display_window="auto"),
    dict(ome_metadata=True, display_window=(1.0,)),
    dict(ome_metadata=True, display_window=(1.0, 2.0, 3.0)),
    dict(ome_metadata=True, display_window=("a", "b")),
    dict(ome_metadata=True, display_window=5),
    dict(ome_metadata=True, voxel_size=None),
    dict(ome_metadata=True, voxel_size=(2.0, 1.8)),
    dict(ome_metadata=True, voxel_size=(2.0, 0.0, 1.8)),
    dict(ome_metadata=True, voxel_size=(2.0, -1.0, 1.8)),
    dict(ome_metadata=True, voxel_size=("a", 1.0, 1.8)),
    dict(ome_metadata=True, image_name=None),
    dict(ome_metadata=True, image_name=7),
])  # fmt: skip
def test_compute_multiscale_option_errors_come_before_anything_is_written(tmp_path, kw):
    g = _level0(tmp_path)
    before = sorted(os.listdir(g))
    with pytest.raises(ValueError):
        _multiscale(g, **kw)
    assert sorted(os.listdir(g)) == before == ["0"]  # no level, no .zattrs, no .zgroup


def _tile(tmp_path):
    src = str(tmp_path / "in" / "X_0_Y_0.zarr")
    MiniZarrArray.create(os.path.join(src, "0"), (1, 1, 8, 32, 48), (1, 1, 4, 16, 16), np.uint16, compressor=None)
    return src, str(tmp_path / "out" / "X_0_Y_0.zarr")


def _destripe_zarr(src, out, xyz=(1.8, 1.8, 2.0), **kw):
    from aind_smartspim_destripe_amd import synth

    return zd.destripe_zarr(src, "0", out, (4, 32, 48), 3072, 0, 1, (8, 32, 48), os.path.dirname(out),
                            os.path.join(os.path.dirname(out), "no_derivatives"), xyz,
                            {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG},
                            output_chunks=(1, 1, 4, 16, 16), **kw)  # fmt: skip


class _BarrierOnly:
    def barrier(self):
        raise AssertionError("nothing may be created or awaited before the options are checked")


@pytest.mark.parametrize("kw", [
    dict(display_window=(0.0, 10.0)),
    dict(display_window="percentile"),
    dict(ome_metadata=True, display_window="auto"),
    dict(ome_metadata=True, display_window=(1.0,)),
    dict(ome_metadata=True, xyz=None),
    dict(ome_metadata=True, xyz=(1.8, 1.8)),
    dict(ome_metadata=True, xyz=(1.8, 0.0, 2.0)),
    dict(ome_metadata=True, display_window="percentile", world_size=2, rank=1, group=_BarrierOnly()),  # no sum_counts
    dict(ome_metadata=True, display_window="percentile", world_size=2, rank=0, group=None),
])  # fmt: skip
def test_destripe_zarr_option_errors_come_before_anything_is_created(tmp_path, kw):
    src, out = _tile(tmp_path)
    with pytest.raises(ValueError):
        _destripe_zarr(src, out, **kw)
    assert not os.path.exists(os.path.dirname(out))


def test_destripe_channel_option_errors_come_before_anything_is_created(tmp_path):
    from aind_smartspim_destripe_amd import synth

    root, results = tmp_path / "data", tmp_path / "results"
    MiniZarrArray.create(str(root / "Ex_488_Em_525" / "X_0_Y_0.zarr" / "0"), (1, 1, 8, 32, 48), (1, 1, 4, 16, 16),
                         np.uint16, compressor=None)  # fmt: skip
    params = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
    for kw in (dict(display_window=(0.0, 10.0)), dict(display_window="percentile"),
               dict(ome_metadata=True, display_window="percentile", world_size=2, group=_BarrierOnly())):  # fmt: skip
        with pytest.raises(ValueError):
            zd.destripe_channel(str(root), str(tmp_path / "derivatives"), "Ex_488_Em_525", str(results), (1.8, 1.8, 2.0),
                                {0: "flat0.tif"}, {0: ["X_0_Y_0"]}, params, **kw)  # fmt: skip
        assert not results.exists()


def test_store_refuses_a_histogram_of_the_wrong_kind_before_anything_is_created(tmp_path):
    from aind_smartspim_destripe_amd import synth

    src, out = _tile(tmp_path)
    for hist in (np.zeros(65536, np.int32), np.zeros(65535, np.int64), np.zeros((2, 65536), np.int64)[:, ::2], [0] * 65536):
        with pytest.raises(ValueError):
            zd.destripe_zarr_store(os.path.join(src, "0"), os.path.join(out, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                   prediction_chunksize=(4, 32, 48), output_chunks=(1, 1, 4, 16, 16), histogram=hist)  # fmt: skip
    assert not os.path.exists(os.path.dirname(out))


# ---- RankGroup.sum_counts ---------------------------------------------------------------------------------------------
class _NoRcclEngine:
    """An engine whose communicator cannot be built: the group falls back to the host transport (files)."""

    def comm_unique_id(self):
        return b"\0" * 128

    def comm_init(self, *a):
        raise OSError("no RCCL here")

    def comm_destroy(self):
        pass


def _counts(rank):
    c = np.zeros(65536, np.int64)
    c[rank] = 1 + rank
    c[65535] = (1 << 40) + rank  # above 2^32 and above what a double-free sum would need
    c[1000:1010] = np.arange(10) * (rank + 1)
    return c


def _sum_counts_worker(rank, world, xdir, q):
    sys.path.insert(0, REPO)
    from aind_smartspim_destripe_amd import distributed as dd

    grp = dd.RankGroup(_NoRcclEngine(), rank, world, dd.FileRendezvous(rank, world, xdir, timeout=60.0))
    first = grp.sum_counts(_counts(rank))
    second = grp.sum_counts(np.full(4, rank + 1, np.int64))  # a second call does not read the first one's keys
    transport = grp.transport
    grp.close()
    q.put((rank, transport, first.dtype.str, first.tobytes(), second.tolist()))


def test_sum_counts_two_ranks_over_the_host_transport(tmp_path):
    import multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sum_counts_worker, args=(r, world, str(tmp_path / "rdzv"), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _counts(0) + _counts(1)
    for rank, transport, dtype, raw, second in res:
        assert transport == "host" and dtype == "<i8"
        assert np.array_equal(np.frombuffer(raw, np.int64), want), rank
        assert second == [3, 3, 3, 3]


def test_sum_counts_of_one_rank_is_the_input():
    from aind_smartspim_destripe_amd import distributed as dd

    grp = dd.RankGroup(_NoRcclEngine(), 0, 1)
    assert not grp.active
    c = _counts(3)
    assert np.array_equal(grp.sum_counts(c), c)
