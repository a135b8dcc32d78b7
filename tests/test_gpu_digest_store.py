"""GPU: digest manifests from the store pass, and reading stores back against them.  The store-matrix geometry
(``store_matrix_cases.py``: 22 x 70 x 100, output chunks (4, 32, 32), z blocks of 8 / 8 / 6 planes, the last ending inside a
chunk) through ``destripe_zarr_store(digests=True)`` and ``compute_multiscale(digests=True)`` on every route.  Every pass
runs once with the option and once without (module fixtures); the tests compare what the two left behind."""

import os
import shutil
import struct

import numpy as np
import pytest

import digest_cases as dc
from aind_smartspim_destripe_amd import integrity, pyramid
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import DIGEST_BIN, DIGEST_JSON, MiniZarrArray
from tests import store_matrix_cases as sm

pytestmark = pytest.mark.gpu

SIDECARS = {DIGEST_JSON, DIGEST_BIN}
# name: (output compressor, device_codec, device_decode, fused pyramid scale or None, block z)
PASSES = {
    "raw-retile": (None, False, False, None, 8),
    "zstd-runs-decode-fused222": ("blosc", "runs", True, (2, 2, 2), 8),
    "zstd-runs-decode-fused122": ("blosc", "runs", True, (1, 2, 2), 4),
    "lz4-device-codec": (sm.LZ4, True, False, None, 8),
}


def _store(tile, group, name, digests):
    out, codec, decode, scale, bz = PASSES[name]
    n, _ = zd.destripe_zarr_store(
        os.path.join(tile, "0"), os.path.join(group, "0"), sm.CELLS, sm.NO_CELLS, None, prediction_chunksize=(bz, sm.H, sm.W),
        output_chunks=sm.OUT_CHUNKS, device=0, compressor=out, device_retile=True, io_threads=4, device_codec=codec,
        device_decode=decode, pyramid_group=group if scale else None, n_levels=3 if scale else 1,
        scale_factor=scale or (2, 2, 2), digests=digests)  # fmt: skip
    assert n == sm.Z and zd.LAST_RUN["digests"] is digests
    assert zd.LAST_RUN["pyramid_levels"] == ([1, 2] if scale else [])


@pytest.fixture(scope="module")
def tile(tmp_path_factory):
    return sm.write_input(tmp_path_factory.mktemp("digest_in"), "blosc")


@pytest.fixture(scope="module")
def stores(tmp_path_factory, tile):
    """``{pass name: (group written with digests, group written without)}``, every pass run once each way."""
    made = {}
    for name in PASSES:
        root = tmp_path_factory.mktemp("digest_" + name)
        made[name] = (str(root / "on" / "t.zarr"), str(root / "off" / "t.zarr"))
        _store(tile, made[name][1], name, False)
        _store(tile, made[name][0], name, True)
    zd.release_staging()
    return made


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _arrays(group):
    return [os.path.join(group, d) for d in sorted(os.listdir(group), key=int)]


def _check_pair(on, off, n_arrays):
    """The option adds the two sidecar files per array and changes no other byte; without it no sidecar exists."""
    assert not [f for f in _files(off) if os.path.basename(f) in SIDECARS]
    extra = sorted(set(_files(on)) - set(_files(off)))
    assert extra == sorted(os.path.join(str(lvl), s) for lvl in range(n_arrays) for s in SIDECARS)
    assert set(_files(off)) <= set(_files(on))
    for rel in _files(off):  # .zarray and every chunk file
        with open(os.path.join(on, rel), "rb") as a, open(os.path.join(off, rel), "rb") as b:
            assert a.read() == b.read(), rel


def _check_manifests(group):
    """Every array's manifest is the restatement of the voxels the host decoders read back."""
    for p in _arrays(group):
        arr = MiniZarrArray.open(p)
        assert arr.digest_grid is not None, p
        vol = arr[0, 0]
        assert vol.any()
        assert dc.as_triples(arr.digest_records()) == dc.restate_array(vol, arr.chunks[-3:]), p


@pytest.mark.parametrize("name", list(PASSES))
def test_store_pass_manifest(stores, name):
    on, off = stores[name]
    n_arrays = 3 if PASSES[name][3] else 1
    assert len(_arrays(on)) == n_arrays
    _check_pair(on, off, n_arrays)
    _check_manifests(on)


def _corrupt(arr_path, n):
    """Swap chunk ``n`` of the array for its neighbour's valid file (the voxels differ: the filter's output is no
    constant); returns what to call to put it back."""
    arr = MiniZarrArray.open(arr_path)
    grid = arr.digest_grid
    path = lambda k: arr._chunk_path((0, 0) + tuple(int(i) for i in np.unravel_index(k, grid)))  # noqa: E731
    keep = path(n) + ".keep"
    shutil.copy(path(n), keep)
    shutil.copy(path(n + 1), path(n))
    return lambda: os.replace(keep, path(n))


DECODES = [False, True, "any"]


def _check_readback(on, decode):
    """``verify_store`` with ``device_decode=decode`` is clean on the group (or array) ``on`` and, with one chunk file of
    its last array swapped for a neighbour's, names exactly that chunk."""
    rep = integrity.verify_store(on, device_decode=decode, io_threads=4, device=0)
    assert rep["bad"] == [] and rep["arrays"] == len(_arrays(on))
    assert rep["chunks"] == sum(int(np.prod(MiniZarrArray.open(p).digest_grid)) for p in _arrays(on))
    target = _arrays(on)[-1]
    n = 0 if int(np.prod(MiniZarrArray.open(target).digest_grid)) > 1 else None
    if n is None:  # (the last level of a small pyramid is one chunk wide: damage level 0 instead)
        target, n = _arrays(on)[0], 40
    restore = _corrupt(target, n)
    try:
        rep = integrity.verify_store(on, device_decode=decode, io_threads=4, device=0)
    finally:
        restore()
    assert rep["bad"] == [(target, n, "digest")]
    assert np.array_equal(integrity.digest_store(target, device_decode=decode, io_threads=4, device=0),
                          MiniZarrArray.open(target).digest_records())  # fmt: skip


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("decode", DECODES, ids=["host-decode", "device-zstd", "device-any"])
def test_verify_store_reads_it_back(stores, name, decode):
    _check_readback(stores[name][0], decode)


def _set_reserved_bit(path):
    """Set the reserved bit of the first Blosc block's zstd frame header: a mutation the decoders' CPU sanitizer runs
    cover, which libzstd and the device decoder both refuse."""
    with open(path, "rb") as fh:
        frame = bytearray(fh.read())
    pos = struct.unpack("<I", frame[16:20])[0] + 4
    assert frame[pos : pos + 4] == b"\x28\xb5\x2f\xfd"
    frame[pos + 4] |= 0x08
    with open(path, "wb") as fh:
        fh.write(bytes(frame))


def test_every_undecodable_chunk_is_named(stores, tmp_path):
    """Two refused zstd frames in different blocks of the read: both are named, by the device task's status or by the
    host decoder's error.  Then a truncated file as well, which stops the batched read: the block is re-read chunk by
    chunk and all three are named."""
    vol = MiniZarrArray.open(os.path.join(stores["zstd-runs-decode-fused222"][0], "0"))[0, 0]
    arr = MiniZarrArray.create(str(tmp_path / "0"), (1, 1) + vol.shape, sm.OUT_CHUNKS, np.uint16, compressor="blosc", digests=True)
    arr[0, 0] = vol
    path = lambda k: arr._chunk_path((0, 0) + tuple(int(i) for i in np.unravel_index(k, arr.digest_grid)))  # noqa: E731
    for k in (3, 50):
        _set_reserved_bit(path(k))
    for decode in (True, False):
        rep = integrity.verify_store(arr.path, device_decode=decode, io_threads=4, device=0)
        assert rep["bad"] == [(arr.path, 3, "undecodable"), (arr.path, 50, "undecodable")], (decode, rep["bad"])
        assert all(rep["detail"][(arr.path, k)] for k in (3, 50))
        if decode:
            assert "device decode status" in rep["detail"][(arr.path, 3)]
    blob = open(path(20), "rb").read()
    open(path(20), "wb").write(blob[: len(blob) // 2])
    for decode in (True, False):
        rep = integrity.verify_store(arr.path, device_decode=decode, io_threads=4, device=0)
        assert rep["bad"] == [(arr.path, k, "undecodable") for k in (3, 20, 50)], (decode, rep["bad"])


@pytest.mark.parametrize("route", ["pipelined", "pipelined-device-codecs", "slabs"])
def test_compute_multiscale_manifests(stores, tmp_path, route):
    """The levels of a finished level 0, on the pipelined route (host and device codecs) and on the slab route."""
    level0 = os.path.join(stores["zstd-runs-decode-fused222"][0], "0")
    kw = {"pipelined": dict(pipelined=True, io_threads=4),
          "pipelined-device-codecs": dict(pipelined=True, io_threads=4, device_codec="runs", device_decode=True),
          "slabs": {}}[route]  # fmt: skip
    groups = {}
    for digests in (False, True):
        groups[digests] = str(tmp_path / ("on" if digests else "off"))
        os.makedirs(groups[digests])
        os.symlink(level0, os.path.join(groups[digests], "0"))
        zd.compute_multiscale(level0, groups[digests], [2, 2, 2], 1, None, sm.TILE, n_levels=3, chunks=sm.OUT_CHUNKS,
                              compressor="blosc", device=0, digests=digests, **kw)  # fmt: skip
        assert pyramid.LAST_PYRAMID["digests"] is digests
        assert pyramid.LAST_PYRAMID["route"] == ("slabs" if route == "slabs" else "pipelined")
        os.remove(os.path.join(groups[digests], "0"))
    for lvl in ("1", "2"):
        on, off = os.path.join(groups[True], lvl), os.path.join(groups[False], lvl)
        assert sorted(set(_files(on)) - set(_files(off))) == sorted(SIDECARS) and set(_files(off)) <= set(_files(on))
        for rel in _files(off):
            with open(os.path.join(on, rel), "rb") as a, open(os.path.join(off, rel), "rb") as b:
                assert a.read() == b.read(), (lvl, rel)
        arr = MiniZarrArray.open(on)
        assert dc.as_triples(arr.digest_records()) == dc.restate_array(arr[0, 0], arr.chunks[-3:])
    # the fused pass left the same records for the same levels
    for lvl in ("1", "2"):
        fused = MiniZarrArray.open(os.path.join(stores["zstd-runs-decode-fused222"][0], lvl))
        assert np.array_equal(fused.digest_records(), MiniZarrArray.open(os.path.join(groups[True], lvl)).digest_records())
    for decode in DECODES:  # clean, and a swapped chunk of level 2 is named, on every decode route
        _check_readback(groups[True], decode)


def test_host_path_of_an_odd_sized_volume(tmp_path):
    """Odd planes take the host path of the store pass: the records come from the array's own writes."""
    Z, H, W = 6, 35, 51
    vol = sm.volume()[:Z, :H, :W]
    src = MiniZarrArray.create(str(tmp_path / "in" / "0"), (1, 1, Z, H, W), (1, 1, 3, 24, 40), np.uint16, compressor="blosc")
    src[0, 0] = vol
    for digests in (False, True):
        out = str(tmp_path / ("on" if digests else "off") / "0")
        n, _ = zd.destripe_zarr_store(src.path, out, sm.CELLS, sm.NO_CELLS, None, prediction_chunksize=(4, H, W),
                                      output_chunks=sm.OUT_CHUNKS, device=0, compressor="blosc", io_threads=2,
                                      digests=digests)  # fmt: skip
        assert n == Z and zd.LAST_RUN["digests"] is digests and zd.LAST_RUN["decode_routes"] is None  # the host path
    _check_pair(str(tmp_path / "on"), str(tmp_path / "off"), 1)
    _check_manifests(str(tmp_path / "on"))
    assert MiniZarrArray.open(str(tmp_path / "on" / "0")).digest_grid == (2, 2, 2)  # a ragged last chunk on every axis
    for decode in DECODES:
        _check_readback(str(tmp_path / "on"), decode)


def _destripe_zarr(tile, out, **kw):
    return zd.destripe_zarr(
        tile, "0", out, (sm.BLOCK_Z, sm.H, sm.W), 3072, 0, 1, (384, sm.H, sm.W), os.path.dirname(out), os.path.join(os.path.dirname(out), "no-derivatives"),
        sm.XYZ, {"cells_config": sm.CELLS, "no_cells_config": sm.NO_CELLS}, output_chunks=sm.OUT_CHUNKS, device=0,
        n_levels=3, io_threads=4, device_codec="runs", device_decode=True, **kw)  # fmt: skip


def test_a_torn_manifest_is_reported_and_the_other_arrays_are_still_checked(stores, tmp_path):
    group = str(tmp_path / "t.zarr")
    shutil.copytree(stores["zstd-runs-decode-fused222"][0], group)
    with open(os.path.join(group, "1", DIGEST_BIN), "r+b") as f:
        f.truncate(100)  # not a whole number of records, and not the grid's
    _corrupt(os.path.join(group, "2"), 0)
    for decode in (False, True):
        rep = integrity.verify_store(group, device_decode=decode, io_threads=4, device=0)
        assert rep["arrays"] == 3 and rep["chunks"] == 72 + 2
        assert rep["bad"] == [(os.path.join(group, "1"), None, "bad manifest"), (os.path.join(group, "2"), 0, "digest")]
        assert rep["detail"][(os.path.join(group, "1"), None)]


@pytest.mark.parametrize("pyr", ["fused", "pipelined", "slabs"])
def test_destripe_zarr_verify(tile, tmp_path, monkeypatch, pyr):
    kw = {"fused": dict(fused_pyramid=True), "pipelined": dict(pipelined_pyramid=True), "slabs": {}}[pyr]
    out = str(tmp_path / "good" / (sm.TILE + ".zarr"))
    _destripe_zarr(tile, out, verify=True, **kw)
    rep = zd.LAST_RUN["verify"]
    assert zd.LAST_RUN["digests"] is True and rep["bad"] == [] and rep["arrays"] == 3 and rep["chunks"] == 72 + 12 + 2  # 6x3x4, 3x2x2, 2x1x1
    _check_manifests(out)
    plain = str(tmp_path / "plain" / (sm.TILE + ".zarr"))
    _destripe_zarr(tile, plain, **kw)
    assert zd.LAST_RUN["verify"] is None and zd.LAST_RUN["digests"] is False
    _check_pair(out, plain, 3)

    # a chunk file swapped between the write and the verification (the hook lives here, not in the product)
    real = integrity.verify_store

    def swapped(path, **kwargs):
        _corrupt(os.path.join(str(path), "1"), 5)
        return real(path, **kwargs)

    monkeypatch.setattr(integrity, "verify_store", swapped)
    bad = str(tmp_path / "bad" / (sm.TILE + ".zarr"))
    with pytest.raises(ValueError, match="verify: 1 of 86 chunks") as e:
        _destripe_zarr(tile, bad, verify=True, **kw)
    assert "chunk 5: digest" in str(e.value)
    assert zd.LAST_RUN["verify"]["bad"] == [(os.path.join(bad, "1"), 5, "digest")]
    zd.release_staging()
