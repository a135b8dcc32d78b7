"""GPU: the store matrix.  The options of the Zarr store pass driven together through ``destripe_zarr_store`` (and the
first six cases through ``destripe_zarr``) over the 22 x 70 x 100 volume of ``store_matrix_cases.py``, which no chunk
divides: every case checks level 0 against the per-plane API bit for bit and against the NumPy references of the suite
on the sampled planes, and the pyramid, the histogram, the projections, the display window and every chunk file against
NumPy of the level 0 the store holds.  One more test reuses the cached staging buffers and engines between cases."""

import json
import os
import time

import numpy as np
import pytest

from aind_smartspim_destripe_amd import mini_tiff
from aind_smartspim_destripe_amd import projections as pr
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from tests import store_matrix_cases as sm

pytestmark = pytest.mark.gpu

ZYX = (sm.Z, sm.H, sm.W)
PARAMS = {"cells_config": sm.CELLS, "no_cells_config": sm.NO_CELLS}
DECODE_MODES = {False: None, True: "zstd", "any": "any", "full": "full"}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """One input tile per input compressor, written on first use."""
    made = {}

    def get(case):
        comp = sm.in_compressor(case)
        key = json.dumps(comp)
        if key not in made:
            made[key] = sm.write_input(tmp_path_factory.mktemp("matrix_in"), comp)
        return made[key]

    return get


@pytest.fixture(scope="module")
def exact():
    """The per-plane API's level 0 per filter configuration, computed once and frozen."""
    made = {}

    def get(case):
        key = sm.exact_key(case)
        if key not in made:
            made[key] = sm.exact_level0(case)
            assert made[key].shape == ZYX and made[key].dtype == np.uint16
            made[key].setflags(write=False)
        return made[key]

    return get


@pytest.fixture(scope="module")
def independent():
    """The NumPy reference of a sampled plane per filter configuration, computed once."""
    made = {}

    def get(case, z):
        key = sm.exact_key(case) + (z,)
        if key not in made:
            made[key] = sm.independent_plane(case, sm.effective_volume()[z])
        return made[key]

    return get


@pytest.fixture(autouse=True)
def _release():
    yield
    zd.release_staging()


def _projections(case):
    return {key: pr.VolumeProjections(ZYX) for key in (("output", "input") if case.proj == "both" else ("output",))}


def _run_store(case, tile, group, hist=None, proj=None):
    """The case through ``destripe_zarr_store``, rank by rank in this process; the pipelined pyramid afterwards, as
    ``destripe_zarr`` orders it.  Returns what every rank's ``LAST_RUN`` said."""
    fused = case.pyramid == "fused"
    runs, planes = [], 0
    for rank in range(case.ranks):
        n, _ = zd.destripe_zarr_store(
            os.path.join(tile, "0"), os.path.join(group, "0"), sm.CELLS, sm.NO_CELLS, sm.shadow_correction(case),
            prediction_chunksize=(sm.block_z(case), sm.H, sm.W), output_chunks=sm.OUT_CHUNKS, rank=rank,
            world_size=case.ranks, device=0, compressor=case.out, device_retile=case.retile, io_threads=4,
            device_codec=case.codec, device_decode=case.decode, pyramid_group=group if fused else None,
            n_levels=case.n_levels if fused else 1, scale_factor=case.scale or (2, 2, 2), histogram=hist,
            projections=proj, **sm.store_kwargs(case))  # fmt: skip
        planes += n
        runs.append(dict(zd.LAST_RUN, planes=n))
    assert planes == sm.Z
    if case.pyramid == "pipelined":
        out_is_blosc = case.out == "blosc" or isinstance(case.out, dict)
        zd.compute_multiscale(os.path.join(group, "0"), group, list(case.scale), 1, None, sm.TILE, n_levels=case.n_levels,
                              chunks=sm.OUT_CHUNKS, compressor=case.out, device=0, pipelined=True, device_codec=case.codec,
                              device_decode=case.decode if out_is_blosc else False, io_threads=4)  # fmt: skip
    return runs


def _check_runs(case, runs):
    """What every rank resolved to: its z range, its filter and routes, and where its input chunks were decoded."""
    ranges = sm.rank_ranges(case)
    for rank, run in enumerate(runs):
        z0, z1 = ranges[rank]
        assert tuple(run["z_range"]) == (z0, z1) and run["planes"] == z1 - z0, (case.name, rank, run["z_range"])
        assert run["filter"] == case.filter and run["streaks_route"] == case.route and run["rotate"] is case.rotate
        assert run["device_codec_mode"] == sm.codec_mode(case) and run["device_decode_mode"] == DECODE_MODES[case.decode]
        assert run["pyramid_levels"] == ([1, 2] if case.pyramid == "fused" else [])
        assert run["pyramid_scale"] == (case.scale if case.pyramid == "fused" else None)
        assert run["histogram_voxels"] == ((z1 - z0) * sm.H * sm.W if case.hist else None)
        assert run["projections"] == case.proj and run["projection_planes"] == z1 - z0
        if case.filter == "streaks":
            assert run["streaks_shading"] is case.shading
        routes = run["decode_routes"]
        if not case.retile:
            assert routes is None  # the host path reads through the array
            continue
        print("[store matrix] {} rank {}: filter {} route device z_range {} decode_routes {} levels {}".format(
            case.name, rank, case.filter, (z0, z1), routes, [0] + run["pyramid_levels"]))  # fmt: skip
        reads, fill = sm.expected_decode_routes(case, (z0, z1))
        assert routes["fill"] == fill and sum(routes.values()) == reads, (case.name, rank, routes, reads, fill)
        # with device_decode every frame here is of a kind the mode takes; without it none goes to the device
        assert routes["host" if case.decode else "device"] == 0, (case.name, rank, routes)
    if not case.retile:
        print("[store matrix] {}: filter {} route host z_range {} decode_routes None levels [0]".format(
            case.name, case.filter, ranges))  # fmt: skip


def _check_level0(case, level0, exact, independent):
    assert level0.shape == ZYX and level0.dtype == np.uint16
    want = exact(case)
    bad = np.flatnonzero((level0 != want).reshape(sm.Z, -1).any(axis=1))
    assert bad.size == 0, (case.name, "planes that are not the per-plane API's", bad.tolist())
    assert not np.array_equal(level0, sm.effective_volume())  # the filter ran
    for z in sm.SAMPLED:
        ref, tol = independent(case, z)
        d = np.abs(level0[z].astype(np.int64) - ref.astype(np.int64))
        print("[store matrix] {} plane {}: max |store - reference| = {} of {}".format(case.name, z, int(d.max()), tol))
        assert d.max() <= tol, (case.name, z, int(d.max()), int((d > tol).sum()))


def _check_arrays(case, group, level0):
    """Every level: its shape and chunks, its voxels, and every chunk file -- present, whole, and the expected brick with
    the fill value 0 outside the array -- and no file besides."""
    volumes = [level0] + sm.expected_levels(level0, case)
    geometry = [(ZYX, sm.OUT_CHUNKS[-3:])] + sm.level_geometry(case.scale, case.n_levels) if case.pyramid else [(ZYX, sm.OUT_CHUNKS[-3:])]
    assert sorted(d for d in os.listdir(group) if not d.startswith(".")) == [str(i) for i in range(len(volumes))]
    for lvl, (vol, (shape, chunks)) in enumerate(zip(volumes, geometry)):
        arr = MiniZarrArray.open(os.path.join(group, str(lvl)))
        assert arr.shape == (1, 1) + shape and arr.chunks == (1, 1) + chunks and arr.dtype == np.uint16, (case.name, lvl)
        assert arr.compressor_meta == MiniZarrArray._compressor_meta(case.out), (case.name, lvl)
        if lvl:
            assert np.array_equal(arr[0, 0], vol), (case.name, "level", lvl)
        bricks = sm.expected_bricks(vol, chunks)
        files = sorted(os.path.relpath(os.path.join(d, f), arr.path) for d, _, fs in os.walk(arr.path) for f in fs)
        want = sorted([".zarray"] + [os.path.relpath(arr._chunk_path((0, 0) + idx), arr.path) for idx in bricks])
        assert files == want, (case.name, lvl)
        for idx, brick in bricks.items():
            got = arr._read_chunk((0, 0) + idx)[0, 0]  # the host reader (dsx_blosc_decode / zlib / raw)
            assert np.array_equal(got, brick), (case.name, "level", lvl, "chunk", idx)


def _same(got, want, what):
    assert set(got) == set(want) == set(pr.NAMES)
    for k in pr.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)


def _check_products(case, level0, hist, proj):
    if case.hist:
        want = sm.expected_histogram(level0)
        assert int(hist.sum()) == 22 * 70 * 100 and np.array_equal(hist, want), case.name
        assert zd.display_window_from_histogram(hist) == sm.expected_window(level0)
    assert all(p.added.all() for p in proj.values())
    _same(proj["output"].arrays, pr.project_volume(level0), (case.name, "output"))
    if case.proj == "both":
        _same(proj["input"].arrays, pr.project_volume(sm.effective_volume()), (case.name, "input"))


@pytest.mark.parametrize("case", sm.CASES, ids=[c.name for c in sm.CASES])
def test_store_case(tmp_path, inputs, exact, independent, case):
    t0 = time.perf_counter()
    group = str(tmp_path / (sm.TILE + ".zarr"))
    hist = np.zeros(65536, np.int64) if case.hist else None
    proj = _projections(case)
    runs = _run_store(case, inputs(case), group, hist, proj)
    t_run = time.perf_counter() - t0
    _check_runs(case, runs)
    level0 = MiniZarrArray.open(os.path.join(group, "0"))[0, 0]
    _check_level0(case, level0, exact, independent)
    _check_arrays(case, group, level0)
    _check_products(case, level0, hist, proj)
    print("[store matrix] {}: store pass {:.2f} s, case {:.2f} s".format(case.name, t_run, time.perf_counter() - t0))


ENTRY = [c for c in sm.CASES if c.entry]


@pytest.mark.parametrize("case", ENTRY, ids=[c.name for c in ENTRY])
def test_entry_point_case(tmp_path, inputs, exact, case):
    """The case through ``destripe_zarr`` with the OME-NGFF metadata, the percentile window and the QC projections."""
    results = tmp_path / "results"
    group = str(results / (sm.TILE + ".zarr"))
    derivatives, flat = tmp_path / "no_derivatives", None
    if case.shading:
        flat, dark = sm.shading()
        derivatives = tmp_path / "derivatives"
        derivatives.mkdir()
        mini_tiff.imwrite(str(derivatives / "DarkMaster_cropped.tif"), dark.astype(np.uint16))
    n, _ = zd.destripe_zarr(
        inputs(case), "0", group, (sm.block_z(case), sm.H, sm.W), 3072, 0, 1, ZYX, str(results), str(derivatives), sm.XYZ,
        PARAMS, flatfield=flat, device=0, compressor=case.out, output_chunks=sm.OUT_CHUNKS, n_levels=case.n_levels,
        io_threads=4, device_retile=True, device_codec=case.codec, device_decode=case.decode,
        fused_pyramid=case.pyramid == "fused", pipelined_pyramid=case.pyramid == "pipelined", ome_metadata=True,
        display_window="percentile", scale_factor=case.scale, qc_projections=case.proj, **sm.store_kwargs(case))  # fmt: skip
    assert n == sm.Z and zd.LAST_RUN["filter"] == case.filter and zd.LAST_RUN["rotate"] is case.rotate
    assert zd.LAST_RUN["histogram_voxels"] == 22 * 70 * 100
    level0 = MiniZarrArray.open(os.path.join(group, "0"))[0, 0]
    assert np.array_equal(level0, exact(case)), case.name
    _check_arrays(case, group, level0)
    # .zattrs: the window of the written voxels and the scale of every level
    with open(os.path.join(group, ".zgroup")) as f:
        assert json.load(f) == {"zarr_format": 2}
    with open(os.path.join(group, ".zattrs")) as f:
        md = json.load(f)
    window = md["omero"]["channels"][0]["window"]
    want = sm.expected_window(level0)
    assert want == zd.display_window_from_histogram(sm.expected_histogram(level0))
    assert (window["start"], window["end"]) == want == tuple(zd.LAST_RUN["display_window"])
    assert (window["min"], window["max"]) == (0.0, 65535.0) and md["omero"]["rdefs"]["defaultZ"] == sm.Z // 2
    datasets = md["multiscales"][0]["datasets"]
    assert [d["path"] for d in datasets] == [str(i) for i in range(case.n_levels)]
    for d, scale in zip(datasets, sm.expected_scales(case)):
        assert d["coordinateTransformations"] == [{"type": "scale", "scale": scale}], (case.name, d["path"])
    # the QC files against NumPy of the store's own level 0 and of the input as a reader sees it
    names = [sm.TILE + "_mip_{}.tif".format(a) for a in "xyz"] + [sm.TILE + "_projections.npz"]
    assert sorted(os.listdir(str(results))) == sorted([sm.TILE + ".zarr"] + names)
    want_out, want_in = pr.project_volume(level0), pr.project_volume(sm.effective_volume())
    with np.load(str(results / (sm.TILE + "_projections.npz"))) as f:
        both = case.proj == "both"
        assert sorted(f.files) == sorted(list(pr.NAMES) + (["in_" + k for k in pr.NAMES] + ["stripe_gain"] if both else []))
        for k in pr.NAMES:
            assert f[k].dtype == want_out[k].dtype and np.array_equal(f[k], want_out[k]), (case.name, k)
            if both:
                assert f["in_" + k].dtype == want_in[k].dtype and np.array_equal(f["in_" + k], want_in[k]), (case.name, k)
        if both:  # stripes down the columns: the gain is taken over the column sums
            name = "sum_y" if case.rotate else "sum_x"
            gain = f["stripe_gain"]
            assert gain.dtype == np.float32 and gain.shape == ((sm.Z, sm.W) if case.rotate else (sm.Z, sm.H))
            assert (want_in[name] != 0).all()
            assert np.array_equal(gain, want_out[name].astype(np.float32) / want_in[name].astype(np.float32))
    for axis in "zyx":
        img = mini_tiff.imread(str(results / (sm.TILE + "_mip_{}.tif".format(axis))))
        assert img.dtype == np.uint16 and np.array_equal(img, want_out["max_" + axis]), (case.name, axis)


def _files(path):
    out = {}
    for d, _, fs in os.walk(path):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), path)] = fh.read()
    return out


def test_cached_staging_and_engines_between_cases(tmp_path, inputs, exact):
    """Case 2, the same without the histogram and the projections (options outside the cache key: the staging buffers
    are the same object), case 3, then case 2 again into a fresh output: byte for byte the first run's chunk files,
    histogram and projections.  Then the same once more after ``release_staging()``."""
    two, three = sm.BY_NAME["02-stripes-rot-fused122"], sm.BY_NAME["03-stripes-rot-pipelined212"]

    def run(case, name, products=True):
        group = str(tmp_path / name / (sm.TILE + ".zarr"))
        hist = np.zeros(65536, np.int64) if case.hist and products else None
        proj = _projections(case) if products else None
        _run_store(case, inputs(case), group, hist, proj)
        return _files(group), hist, proj

    first, hist, proj = run(two, "a")
    assert len(first) > 3 and np.array_equal(MiniZarrArray.open(str(tmp_path / "a" / (sm.TILE + ".zarr") / "0"))[0, 0], exact(two))
    blocks = zd._BLOCKS["blocks"][1]
    bare, _, _ = run(two, "bare", products=False)
    assert zd._BLOCKS["blocks"][1] is blocks  # reused
    assert sorted(bare) == sorted(first) and [k for k in first if first[k] != bare[k]] == []
    other, _, _ = run(three, "b")
    assert zd._BLOCKS["blocks"][1] is not blocks  # case 3 has another z block and other codecs
    level0 = MiniZarrArray.open(str(tmp_path / "b" / (sm.TILE + ".zarr") / "0"))[0, 0]
    assert np.array_equal(level0, exact(three))
    for name in ("c", "d"):
        again, hist2, proj2 = run(two, name)
        assert sorted(again) == sorted(first) and [k for k in first if first[k] != again[k]] == [], name
        assert np.array_equal(hist2, hist), name
        for key in proj:
            _same(proj2[key].arrays, proj[key].arrays, (name, key))
        zd.release_staging()
        assert "blocks" not in zd._BLOCKS
