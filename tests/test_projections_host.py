"""The QC projections without a GPU: the host build (``dsx_project_u16_ref`` / ``engine.project_ref``;
``csrc/dsx_project.h``) against NumPy, its argument rules, the same code built with g++ from
``tests/host/project_check.cpp`` under ASan / UBSan as its own process, ``projections.VolumeProjections`` and its files,
``RankGroup.reduce_array`` over two processes, and the option rules of the three entry points."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import projection_cases as pc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_tiff, synth
from aind_smartspim_destripe_amd import projections as pr
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DSX_EINVAL, DSX_ELIMIT = -1, -5
CASES = pc.cases()


def _same(got, want):
    assert set(got) == set(want) == set(pr.NAMES)
    for k in pr.NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name,buf,z0,nz", CASES, ids=[c[0] for c in CASES])
def test_project_ref_is_project_volume(name, buf, z0, nz):
    got = eng_mod.project_ref(buf[z0 : z0 + nz])
    _same(got, pc.expected(name))
    if name.startswith("d_"):
        assert got["max_z"].max() < 60000  # nothing on either side of the range was read
    if name == "c_constant_65535":
        assert got["sum_x"][0, 0] == 128 * 65535 and got["sum_y"][0, 0] == 64 * 65535 and got["sum_z"][0, 0] == 4 * 65535


@pytest.mark.parametrize("vol", [pc.seven_planes(), pc.wide_seven()], ids=["odd", "wide"])
def test_project_ref_accumulates_over_blocks(vol):
    """Blocks of 4 and 3 planes equal the 7-plane volume; the rows outside [z_off, z_off + Z) keep their canary."""
    acc = pc.canary_arrays((9,) + vol.shape[1:])  # two rows more than the volume: row 0 and row 8 are never written
    assert eng_mod.project_ref(vol[:4], acc=acc, z_off=1) is acc
    for k, c in pc.CANARY.items():
        assert (acc[k][0] == c).all() and (acc[k][5:] == c).all(), k
    _same({k: (a if k.endswith("_z") else a[1:5]) for k, a in acc.items()}, pr.project_volume(vol[:4]))
    eng_mod.project_ref(vol[4:], acc=acc, z_off=5)
    for k, c in pc.CANARY.items():
        assert (acc[k][0] == c).all() and (acc[k][8] == c).all(), k
    _same({k: (a if k.endswith("_z") else a[1:8]) for k, a in acc.items()}, pr.project_volume(vol))


def test_project_ref_argument_rules():
    lib = eng_mod.load_library()
    vol = np.ascontiguousarray(pc.odd_permutation())
    arrays = {name: np.zeros(shape, dtype) for name, shape, dtype in eng_mod.projection_shapes(vol.shape)}
    table = eng_mod._Projection(*[arrays[n].ctypes.data for n in pr.NAMES])
    vp, tp = vol.ctypes.data_as(ctypes.c_void_p), ctypes.byref(table)
    Z, H, W = vol.shape
    assert lib.dsx_project_u16_ref(None, 0, H, W, None, 0, 1) == 0  # Z == 0 is a no-op, whatever the pointers
    assert lib.dsx_project_u16_ref(None, Z, H, W, tp, 0, 1) == DSX_EINVAL
    assert lib.dsx_project_u16_ref(vp, Z, H, W, None, 0, 1) == DSX_EINVAL
    assert lib.dsx_project_u16_ref(ctypes.c_void_p(vol.ctypes.data + 1), 1, H, W, tp, 0, 1) == DSX_EINVAL  # odd pointer
    for bad in ((-1, H, W, 0), (Z, 0, W, 0), (Z, H, -3, 0), (Z, H, W, -1)):
        assert lib.dsx_project_u16_ref(vp, *bad[:3], tp, bad[3], 1) == DSX_EINVAL, bad
    assert lib.dsx_project_u16_ref(vp, 1, 65537, 1, tp, 0, 1) == DSX_ELIMIT
    assert lib.dsx_project_u16_ref(vp, 1, 1, 65537, tp, 0, 1) == DSX_ELIMIT
    for name in pr.NAMES:  # a NULL member of the table
        hole = eng_mod._Projection(*[None if n == name else arrays[n].ctypes.data for n in pr.NAMES])
        assert lib.dsx_project_u16_ref(vp, Z, H, W, ctypes.byref(hole), 0, 1) == DSX_EINVAL, name
    assert not any(a.any() for a in arrays.values())  # no refused call wrote anything
    assert lib.dsx_project_u16_ref(vp, Z, H, W, tp, 0, 1) == 0 and int(arrays["sum_z"].sum()) == int(vol.sum(dtype=np.uint64))
    n = ctypes.c_size_t(0)
    assert lib.dsx_project_work_bytes(64, 1600, 2000, ctypes.byref(n)) == 0 and n.value % 16 == 0 and n.value > 0
    assert lib.dsx_project_work_bytes(64, 1600, 2000, None) == DSX_EINVAL
    assert lib.dsx_project_work_bytes(1, 65537, 8, ctypes.byref(n)) == DSX_ELIMIT
    assert lib.dsx_project_work_bytes(64, 1600, 2000, ctypes.byref(n)) == 0
    assert eng_mod.project_work_bytes((64, 1600, 2000)) == n.value
    with pytest.raises(ValueError):
        eng_mod.project_ref(vol.astype(np.int16))
    with pytest.raises(ValueError):
        eng_mod.project_ref(vol[0])
    with pytest.raises(ValueError):
        eng_mod.project_ref(vol, z_off=2)  # z_off counts in acc
    with pytest.raises(ValueError):
        eng_mod.project_ref(vol, acc={**arrays, "sum_z": arrays["sum_z"].astype(np.uint32)})
    with pytest.raises(ValueError):
        eng_mod.project_ref(vol, acc=arrays, z_off=1)  # Z rows do not hold rows 1 .. Z
    with pytest.raises(ValueError):
        eng_mod.project_work_bytes((1, 8, 65537))
    with pytest.raises(ValueError):
        eng_mod.project_ref(np.zeros((1, 1, 65537), np.uint16))


def test_project_host_build_under_sanitizers(tmp_path):
    """tests/host/project_check.cpp with ASan / UBSan on cases (a), (d) and (e): the six arrays, over two calls, and no
    read outside the planes or write outside an array."""
    exe = str(tmp_path / "project_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "project_check.cpp")], check=True)  # fmt: skip
    for name, buf, z0, nz in CASES:
        if name[0] not in "ade":
            continue
        raw, out = str(tmp_path / (name + ".raw")), str(tmp_path / (name + ".out"))
        buf.tofile(raw)
        _, H, W = buf.shape
        res = subprocess.run([exe, raw, str(z0), str(nz), str(H), str(W), out], capture_output=True, text=True)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        blob, at, got = np.fromfile(out, np.uint8), 0, {}
        for k, shape, dtype in eng_mod.projection_shapes((nz, H, W)):
            n = int(np.prod(shape)) * dtype.itemsize
            got[k] = blob[at : at + n].view(dtype).reshape(shape)
            at += n
        assert at == blob.size
        _same(got, pc.expected(name))


# ---- VolumeProjections ---------------------------------------------------------------------------------------------------
def test_volume_projections_add_and_files(tmp_path):
    vol = pc.seven_planes()
    p = pr.VolumeProjections(vol.shape)
    assert not p.added.any() and all(not a.any() for a in p.arrays.values())
    p.add(4, vol[4:])
    assert p.added.tolist() == [False] * 4 + [True] * 3
    with pytest.raises(ValueError):
        p.add(6, vol[6:])  # a plane twice
    with pytest.raises(ValueError):
        p.add(3, vol[3:5])  # overlaps what is there
    with pytest.raises(ValueError):
        p.add(0, vol[:4, :, :-1])  # another plane shape
    with pytest.raises(ValueError):
        p.add(0, vol[:4].astype(np.int32))
    with pytest.raises(ValueError):
        p.add(-1, vol[:1])
    assert p.added.tolist() == [False] * 4 + [True] * 3  # a refused block leaves no trace
    p.add_projected(0, pr.project_volume(vol[:4]))  # what the device path hands over
    with pytest.raises(ValueError):
        p.add_projected(0, pr.project_volume(vol[:4]))
    assert p.added.all()
    _same(p.arrays, pr.project_volume(vol))
    assert p.sum_x is p.arrays["sum_x"] and p.max_z is p.arrays["max_z"]
    assert p.merge(None) is p  # one rank: every plane once
    half = pr.VolumeProjections(vol.shape)
    half.add(0, vol[:4])
    with pytest.raises(RuntimeError):
        half.merge(None)  # planes 4 .. 6 are missing
    path = str(tmp_path / "p.npz")
    p.save(path)
    q = pr.VolumeProjections.load(path)
    assert q.zyx == p.zyx and np.array_equal(q.added, p.added)
    _same(q.arrays, p.arrays)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 65537)):
        with pytest.raises(ValueError):
            pr.VolumeProjections(bad)


def test_stripe_gain_and_write_qc(tmp_path):
    rs = np.random.RandomState(3)
    vin = rs.randint(1, 4000, (5, 6, 8)).astype(np.uint16)
    vin[2, 3] = 0  # a zero row: gain 1.0
    vin[4, :, 5] = 0  # a zero column, for rotate
    vout = (vin // 2).astype(np.uint16)
    vout[2, 3] = 7  # (whatever the output holds there)
    inp, out = pr.VolumeProjections(vin.shape), pr.VolumeProjections(vout.shape)
    inp.add(0, vin)
    out.add(0, vout)
    g = pr.stripe_gain(inp, out)
    assert g.dtype == np.float32 and g.shape == (5, 6) and g[2, 3] == 1.0
    sx_in, sx_out = vin.sum(2, dtype=np.uint32), vout.sum(2, dtype=np.uint32)
    keep = sx_in != 0
    assert np.array_equal(g[keep], sx_out[keep].astype(np.float32) / sx_in[keep].astype(np.float32))
    gr = pr.stripe_gain(inp, out, rotate=True)
    sy_in, sy_out = vin.sum(1, dtype=np.uint32), vout.sum(1, dtype=np.uint32)
    assert gr.shape == (5, 8) and gr[4, 5] == 1.0
    assert np.array_equal(gr[sy_in != 0], sy_out[sy_in != 0].astype(np.float32) / sy_in[sy_in != 0].astype(np.float32))
    with pytest.raises(ValueError):
        pr.stripe_gain(inp, pr.VolumeProjections((5, 6, 9)))

    folder = tmp_path / "results"
    paths = pr.write_qc(str(folder), "X_0_Y_0", out, inp)
    assert sorted(os.listdir(folder)) == ["X_0_Y_0_mip_x.tif", "X_0_Y_0_mip_y.tif", "X_0_Y_0_mip_z.tif", "X_0_Y_0_projections.npz"]
    assert sorted(os.path.basename(p) for p in paths) == sorted(os.listdir(folder))
    with np.load(str(folder / "X_0_Y_0_projections.npz")) as f:
        assert sorted(f.files) == sorted(list(pr.NAMES) + ["in_" + n for n in pr.NAMES] + ["stripe_gain"])
        for n in pr.NAMES:
            assert np.array_equal(f[n], out.arrays[n]) and np.array_equal(f["in_" + n], inp.arrays[n])
        assert np.array_equal(f["stripe_gain"], g)
    for axis, want in (("z", vout.max(0)), ("y", vout.max(1)), ("x", vout.max(2))):
        img = mini_tiff.imread(str(folder / "X_0_Y_0_mip_{}.tif".format(axis)))
        assert img.dtype == np.uint16 and np.array_equal(img, want)
    only = tmp_path / "only"
    pr.write_qc(str(only), "t", out)
    with np.load(str(only / "t_projections.npz")) as f:
        assert sorted(f.files) == sorted(pr.NAMES)


# ---- RankGroup.reduce_array ----------------------------------------------------------------------------------------------
class _NoRcclEngine:
    """An engine whose communicator cannot be built: the group falls back to the host transport (files)."""

    def comm_unique_id(self):
        return b"\0" * 128

    def comm_init(self, *a):
        raise OSError("no RCCL here")

    def comm_destroy(self):
        pass


def _rank_arrays(rank):
    big = np.zeros((3, 5), np.uint64)
    big[0, 0] = (1 << 40) + rank  # above 2^32
    big[1] = np.arange(5, dtype=np.uint64) * (rank + 1)
    peaks = np.array([[rank, 65535 - rank], [7, 100 * rank]], np.uint16)
    return big, peaks


def _reduce_worker(rank, world, xdir, q):
    sys.path.insert(0, REPO)
    from aind_smartspim_destripe_amd import distributed as dd

    grp = dd.RankGroup(_NoRcclEngine(), rank, world, dd.FileRendezvous(rank, world, xdir, timeout=60.0))
    big, peaks = _rank_arrays(rank)
    total = grp.reduce_array(big, "sum")
    top = grp.reduce_array(peaks, "max")
    second = grp.reduce_array(np.full(4, rank + 1, np.uint32), "sum")  # a second call does not read the first one's keys
    transport = grp.transport
    grp.close()
    q.put((rank, transport, total.dtype.str, total.shape, total.tobytes(), top.dtype.str, top.tolist(), second.tolist()))


def test_reduce_array_two_ranks_over_the_host_transport(tmp_path):
    import multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, str(tmp_path / "rdzv"), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (b0, p0), (b1, p1) = _rank_arrays(0), _rank_arrays(1)
    for rank, transport, dtype, shape, raw, top_dtype, top, second in res:
        assert transport == "host" and dtype == "<u8" and shape == (3, 5) and top_dtype == "<u2"
        assert np.array_equal(np.frombuffer(raw, np.uint64).reshape(shape), b0 + b1), rank
        assert top == np.maximum(p0, p1).tolist()
        assert second == [3, 3, 3, 3]


def test_reduce_array_of_one_rank_is_the_input():
    from aind_smartspim_destripe_amd import distributed as dd

    grp = dd.RankGroup(_NoRcclEngine(), 0, 1)
    assert not grp.active
    big, peaks = _rank_arrays(3)
    assert np.array_equal(grp.reduce_array(big, "sum"), big) and np.array_equal(grp.reduce_array(peaks, "max"), peaks)
    with pytest.raises(ValueError):
        grp.reduce_array(big, "min")
    with pytest.raises(ValueError):
        grp.reduce_array(big.astype(np.float64), "sum")


# ---- option rules of the entry points ------------------------------------------------------------------------------------
def _tile(tmp_path, dtype=np.uint16):
    src = str(tmp_path / "in" / "X_0_Y_0.zarr")
    MiniZarrArray.create(os.path.join(src, "0"), (1, 1, 8, 32, 48), (1, 1, 4, 16, 16), dtype, compressor=None)
    return src, str(tmp_path / "out" / "X_0_Y_0.zarr")


class _BarrierOnly:
    def barrier(self):
        raise AssertionError("nothing may be created or awaited before the options are checked")


def test_store_refuses_bad_projections_before_anything_is_created(tmp_path):
    src, out = _tile(tmp_path)
    good = pr.VolumeProjections((8, 32, 48))
    bads = [good, {"input": good}, {"output": good, "gain": good}, {"output": np.zeros((8, 32, 48), np.uint16)},
            {"output": good, "input": None}, {"output": pr.VolumeProjections((8, 32, 47))},
            {"output": good, "input": pr.VolumeProjections((4, 32, 48))}, "output"]  # fmt: skip
    for bad in bads:
        with pytest.raises(ValueError):
            zd.destripe_zarr_store(os.path.join(src, "0"), os.path.join(out, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                                   prediction_chunksize=(4, 32, 48), output_chunks=(1, 1, 4, 16, 16), projections=bad)  # fmt: skip
    assert not os.path.exists(os.path.dirname(out))
    assert not good.added.any()
    fsrc, fout = _tile(tmp_path / "f32", np.float32)  # an array that is not uint16
    with pytest.raises(ValueError):
        zd.destripe_zarr_store(os.path.join(fsrc, "0"), os.path.join(fout, "0"), synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG,
                               prediction_chunksize=(4, 32, 48), output_chunks=(1, 1, 4, 16, 16),
                               projections={"output": good})  # fmt: skip
    assert not os.path.exists(os.path.dirname(fout))


@pytest.mark.parametrize("kw", [
    dict(qc_projections="input"),
    dict(qc_projections=True),
    dict(qc_projections=["output"]),
    dict(qc_projections="both", world_size=2, rank=1, group=_BarrierOnly()),  # no reduce_array
    dict(qc_projections="output", world_size=2, rank=0, group=None),
])  # fmt: skip
def test_destripe_zarr_refuses_bad_qc_options_before_anything_is_created(tmp_path, kw):
    src, out = _tile(tmp_path)
    with pytest.raises(ValueError):
        zd.destripe_zarr(src, "0", out, (4, 32, 48), 3072, 0, 1, (8, 32, 48), str(tmp_path / "results"),
                         os.path.join(os.path.dirname(out), "no_derivatives"), (1.8, 1.8, 2.0),
                         {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG},
                         output_chunks=(1, 1, 4, 16, 16), **kw)  # fmt: skip
    assert not os.path.exists(os.path.dirname(out)) and not (tmp_path / "results").exists()


def test_destripe_channel_refuses_bad_qc_options_before_anything_is_created(tmp_path):
    root, results = tmp_path / "data", tmp_path / "results"
    MiniZarrArray.create(str(root / "Ex_488_Em_525" / "X_0_Y_0.zarr" / "0"), (1, 1, 8, 32, 48), (1, 1, 4, 16, 16),
                         np.uint16, compressor=None)  # fmt: skip
    params = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
    for kw in (dict(qc_projections="all"), dict(qc_projections=1),
               dict(qc_projections="both", world_size=2, group=_BarrierOnly())):  # fmt: skip
        with pytest.raises(ValueError):
            zd.destripe_channel(str(root), str(tmp_path / "derivatives"), "Ex_488_Em_525", str(results), (1.8, 1.8, 2.0),
                                {0: "flat0.tif"}, {0: ["X_0_Y_0"]}, params, **kw)  # fmt: skip
        assert not results.exists()
