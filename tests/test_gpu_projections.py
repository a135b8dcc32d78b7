"""``k_project_u16`` / ``k_project_fold`` (``csrc/dsx_project.h``) on the device against NumPy, exactly: odd and wide
shapes, constant volumes, unaligned guarded sub-ranges, degenerate shapes, accumulation over blocks, arguments -- and the
``projections`` option of the store pass and ``qc_projections`` of ``destripe_zarr`` on every route."""

import ctypes
import os

import numpy as np
import pytest

import projection_cases as pc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_tiff, synth
from aind_smartspim_destripe_amd import projections as pr
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

DSX_EINVAL, DSX_ELIMIT = -1, -5
CASES = pc.cases()


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _same(got, want):
    assert set(got) == set(want) == set(pr.NAMES)
    for k in pr.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _free(bufs):
    for b in bufs:
        b.free()


@pytest.mark.parametrize("name,buf,z0,nz", CASES, ids=[c[0] for c in CASES])
def test_device_projections_are_project_volume(eng, name, buf, z0, nz):
    _, H, W = buf.shape
    if name.startswith("d_"):
        assert (2 * z0 * H * W) % 16 == 2  # 2-byte aligned only (device allocations are 256-byte aligned)
    d = eng.alloc(max(buf.nbytes, 16))
    bufs = eng.alloc_projection((nz, H, W))
    try:
        d.upload(buf)
        eng.project(d.ptr + 2 * z0 * H * W, (nz, H, W), bufs)
        got = eng.projection_get(bufs, (nz, H, W))
    finally:
        _free([d] + list(bufs.values()))
    _same(got, pc.expected(name))
    if name.startswith("d_"):
        assert got["max_z"].max() < 60000 and got["max_y"].max() < 60000  # nothing on either side of the range was read


@pytest.mark.parametrize("vol", [pc.seven_planes(), pc.wide_seven()], ids=["odd", "wide"])
def test_device_accumulation_over_blocks(eng, vol):
    """Blocks of 4 and 3 planes with ``first`` / ``z_off`` equal the 7-plane volume; ``first`` overwrites what the z
    arrays held; the rows outside [z_off, z_off + Z) keep their canary; one work buffer serves both calls."""
    _, H, W = vol.shape
    zyx = (9, H, W)  # two rows more than the volume: row 0 and row 8 are never written
    start = pc.canary_arrays(zyx)
    start["max_z"][:] = 0x1234
    start["sum_z"][:] = 1 << 50
    d = eng.alloc(vol.nbytes)
    work = eng.alloc(eng_mod.project_work_bytes((4, H, W)))
    bufs = eng.alloc_projection(zyx)
    try:
        d.upload(vol)
        for k, a in start.items():
            bufs[k].upload(a)
        eng.project(d, (4, H, W), bufs, z_off=1, first=True, d_work=work)
        got = eng.projection_get(bufs, zyx)
        for k, c in pc.CANARY.items():
            assert (got[k][0] == c).all() and (got[k][5:] == c).all(), k
        _same({k: (a if k.endswith("_z") else a[1:5]) for k, a in got.items()}, pr.project_volume(vol[:4]))
        eng.project(d.ptr + 2 * 4 * H * W, (3, H, W), bufs, z_off=5, first=False, d_work=work)
        got = eng.projection_get(bufs, zyx)
        for k, c in pc.CANARY.items():
            assert (got[k][0] == c).all() and (got[k][8] == c).all(), k
        _same({k: (a if k.endswith("_z") else a[1:8]) for k, a in got.items()}, pr.project_volume(vol))
    finally:
        _free([d, work] + list(bufs.values()))


def test_device_argument_rules(eng):
    lib, ctx = eng._lib, eng._ctx
    vol = pc.odd_permutation()
    Z, H, W = vol.shape
    d = eng.alloc(vol.nbytes)
    work = eng.alloc(eng_mod.project_work_bytes(vol.shape))
    bufs = eng.alloc_projection(vol.shape)
    try:
        d.upload(vol)
        table = eng_mod._Projection(*[bufs[n].ptr for n in pr.NAMES])
        dp, tp, wp = ctypes.c_void_p(d.ptr), ctypes.byref(table), ctypes.c_void_p(work.ptr)
        assert lib.dsx_project_u16_device(ctx, None, 0, H, W, None, 0, 1, None) == 0  # Z == 0 is a no-op
        assert lib.dsx_project_u16_device(ctx, None, Z, H, W, tp, 0, 1, wp) == DSX_EINVAL
        assert lib.dsx_project_u16_device(ctx, dp, Z, H, W, None, 0, 1, wp) == DSX_EINVAL
        assert lib.dsx_project_u16_device(ctx, dp, Z, H, W, tp, 0, 1, None) == DSX_EINVAL
        assert lib.dsx_project_u16_device(ctx, ctypes.c_void_p(d.ptr + 1), 1, H, W, tp, 0, 1, wp) == DSX_EINVAL
        assert lib.dsx_project_u16_device(ctx, dp, Z, H, W, tp, -1, 1, wp) == DSX_EINVAL
        assert lib.dsx_project_u16_device(ctx, dp, 1, 65537, 1, tp, 0, 1, wp) == DSX_ELIMIT
        for name in pr.NAMES:
            hole = eng_mod._Projection(*[None if n == name else bufs[n].ptr for n in pr.NAMES])
            assert lib.dsx_project_u16_device(ctx, dp, Z, H, W, ctypes.byref(hole), 0, 1, wp) == DSX_EINVAL, name
        with pytest.raises(ValueError):
            eng.project(d.ptr, (1, 65537, 8), bufs)  # before any launch
        with pytest.raises(ValueError):
            eng.project(d.ptr, (1, 8, 65537), bufs)
        with pytest.raises(ValueError):
            eng.project(d, vol.shape, bufs, z_off=-1)
        assert not any(a.any() for a in eng.projection_get(bufs, vol.shape).values())  # no refused call launched
        eng.project(d, vol.shape, bufs, d_work=work)
        _same(eng.projection_get(bufs, vol.shape), pc.expected("a_odd_permutation"))
    finally:
        _free([d, work] + list(bufs.values()))


# ---- the store pass ------------------------------------------------------------------------------------------------------
Z, H, W = 12, 64, 96
CHUNKS = (1, 1, 4, 32, 32)
PARAMS = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}


def _make_input(folder, width=W):
    path = str(folder / "X_0_Y_0.zarr")
    src = MiniZarrArray.create(os.path.join(path, "0"), (1, 1, Z, H, width), CHUNKS, np.uint16, compressor="blosc")
    src[0, 0] = synth.synthetic_stack(Z, H, width, n_unique=4)
    return path


@pytest.fixture(scope="module")
def tile(tmp_path_factory):
    return _make_input(tmp_path_factory.mktemp("proj_in"))


@pytest.fixture(autouse=True)
def _release():
    yield
    zd.release_staging()


def _store(src, out, **kw):
    return zd.destripe_zarr_store(os.path.join(src, "0"), os.path.join(out, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                  None, prediction_chunksize=(4, H, kw.pop("width", W)), output_chunks=CHUNKS, device=0,
                                  io_threads=4, **kw)  # fmt: skip


def _level0(path):
    return MiniZarrArray.open(os.path.join(path, "0"))[0, 0]


def _files(path):
    out = {}
    for d, _, fs in os.walk(path):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), path)] = fh.read()
    return out


@pytest.mark.parametrize("name,kw,pyramid", [
    ("stripes", dict(device_retile=True), False),
    ("streaks", dict(device_retile=True, streaks={"sigma": (8.0, 16.0)}), False),
    ("device_codecs_fused", dict(device_retile=True, device_codec="runs", device_decode=True), True),
    ("rotate", dict(device_retile=True, rotate=True), False),
])  # fmt: skip
def test_store_projections_on_the_device_route(tmp_path, tile, name, kw, pyramid):
    """Three blocks of 4 planes (both buffer sets): the output arrays are those of the written level 0, the input arrays
    those of the source, and the store's files are byte for byte those of the call without the option."""
    plain, with_p = str(tmp_path / "plain.zarr"), str(tmp_path / "proj.zarr")
    n, _ = _store(tile, plain, **kw, **(dict(pyramid_group=plain, n_levels=3) if pyramid else {}))
    assert n == Z and zd.LAST_RUN["projections"] is None and zd.LAST_RUN["projection_planes"] is None
    p = {"output": pr.VolumeProjections((Z, H, W)), "input": pr.VolumeProjections((Z, H, W))}
    n, _ = _store(tile, with_p, projections=p, **kw, **(dict(pyramid_group=with_p, n_levels=3) if pyramid else {}))
    assert n == Z and zd.LAST_RUN["projections"] == "both" and zd.LAST_RUN["projection_planes"] == Z
    assert p["output"].added.all() and p["input"].added.all()
    vol = _level0(with_p)
    assert vol.shape == (Z, H, W)
    _same(p["output"].arrays, pr.project_volume(vol))
    _same(p["input"].arrays, pr.project_volume(_level0(tile)))
    a, b = _files(plain), _files(with_p)
    assert sorted(a) == sorted(b) and len(a) > 1, name
    assert [k for k in a if a[k] != b[k]] == [], name
    only = {"output": pr.VolumeProjections((Z, H, W))}
    _store(tile, with_p, projections=only, **kw, **(dict(pyramid_group=with_p, n_levels=3) if pyramid else {}))
    assert zd.LAST_RUN["projections"] == "output"
    _same(only["output"].arrays, p["output"].arrays)
    with pytest.raises(ValueError):  # the same planes a second time
        _store(tile, with_p, projections=only, **kw, **(dict(pyramid_group=with_p, n_levels=3) if pyramid else {}))


def test_store_projections_on_the_host_route(tmp_path):
    """A 64 x 95 store cannot take the device re-tiling: the chunk map projects what ``execute_worker`` is given and what
    it assigns."""
    src = _make_input(tmp_path, width=95)
    plain, with_p = str(tmp_path / "plain.zarr"), str(tmp_path / "proj.zarr")
    _store(src, plain, width=95)
    p = {"output": pr.VolumeProjections((Z, H, 95)), "input": pr.VolumeProjections((Z, H, 95))}
    n, _ = _store(src, with_p, width=95, projections=p)
    assert n == Z and zd.LAST_RUN["projections"] == "both" and zd.LAST_RUN["projection_planes"] == Z
    assert p["output"].added.all() and p["input"].added.all()
    _same(p["output"].arrays, pr.project_volume(_level0(with_p)))
    _same(p["input"].arrays, pr.project_volume(_level0(src)))
    a, b = _files(plain), _files(with_p)
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == []


def _destripe_zarr(src, out, **kw):
    return zd.destripe_zarr(src, "0", out, (4, H, W), 3072, 0, 1, (Z, H, W), os.path.dirname(out),
                            os.path.join(os.path.dirname(out), "no_derivatives"), (1.8, 1.9, 2.0), PARAMS, device=0,
                            output_chunks=CHUNKS, n_levels=3, io_threads=4, device_retile=True, **kw)  # fmt: skip


def test_destripe_zarr_writes_the_qc_files(tmp_path, tile):
    plain, with_qc = str(tmp_path / "plain" / "X_0_Y_0.zarr"), str(tmp_path / "qc" / "X_0_Y_0.zarr")
    _destripe_zarr(tile, plain)
    assert os.listdir(os.path.dirname(plain)) == ["X_0_Y_0.zarr"]  # without the option the folder is as it was
    n, _ = _destripe_zarr(tile, with_qc, qc_projections="both")
    folder = os.path.dirname(with_qc)
    assert n == Z and sorted(os.listdir(folder)) == ["X_0_Y_0.zarr", "X_0_Y_0_mip_x.tif", "X_0_Y_0_mip_y.tif",
                                                      "X_0_Y_0_mip_z.tif", "X_0_Y_0_projections.npz"]  # fmt: skip
    vol, src = _level0(with_qc), _level0(tile)
    want_out, want_in = pr.project_volume(vol), pr.project_volume(src)
    with np.load(os.path.join(folder, "X_0_Y_0_projections.npz")) as f:
        assert sorted(f.files) == sorted(list(pr.NAMES) + ["in_" + k for k in pr.NAMES] + ["stripe_gain"])
        for k in pr.NAMES:
            assert f[k].dtype == want_out[k].dtype and np.array_equal(f[k], want_out[k]), k
            assert np.array_equal(f["in_" + k], want_in[k]), k
        gain = f["stripe_gain"]
    sx_in, sx_out = want_in["sum_x"], want_out["sum_x"]
    assert gain.dtype == np.float32 and gain.shape == (Z, H) and (sx_in != 0).all()
    assert np.array_equal(gain, sx_out.astype(np.float32) / sx_in.astype(np.float32))
    for axis in "zyx":
        img = mini_tiff.imread(os.path.join(folder, "X_0_Y_0_mip_{}.tif".format(axis)))
        assert img.dtype == np.uint16 and np.array_equal(img, want_out["max_" + axis]), axis
    a, b = _files(plain), _files(with_qc)
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == []
    out_only = str(tmp_path / "out_only" / "X_0_Y_0.zarr")
    _destripe_zarr(tile, out_only, qc_projections="output", fused_pyramid=True)
    with np.load(os.path.join(os.path.dirname(out_only), "X_0_Y_0_projections.npz")) as f:
        assert sorted(f.files) == sorted(pr.NAMES)
        assert np.array_equal(f["sum_z"], pr.project_volume(_level0(out_only))["sum_z"])
