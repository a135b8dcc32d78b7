"""The pipelined stand-alone pyramid without a GPU: the host build of ``dsx_pyramid_bricks_u16``
(``engine.pyramid_bricks_ref``: the pyramid levels of a block that is still in chunk order) against the host build from
the dense block (``engine.pyramid_block_ref``), the padding of the source bricks that must never be read, levels
assembled block by block against the whole-volume pyramid, the block-size helper, the pass itself on a host stand-in for
the device, the new keywords and the refusals that precede engine creation."""

import inspect
import itertools
import os

import numpy as np
import pytest

from aind_smartspim_destripe_amd import engine, pyramid
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import format_oracle as fo

BLOCKS = [(64, 36, 50), (8, 20, 44), (6, 10, 12), (7, 9, 11), (64, 256, 384)]
SRC_CHUNKS = [(64, 128, 128), (4, 8, 8), (3, 5, 7), (2, 16, 24)]
BASES = [(64, 128, 128), (4, 8, 8), (3, 5, 7)]


def level_chunk_cases(zyx):
    """The distinct lists of level chunk shapes of ``test_block_ref_equals_the_oracle``: ``n_levels`` 2 to 5, chunks of a
    volume this block is all of (clamped) and of a taller one (z unclamped); levels with an empty share dropped."""
    seen, out = set(), []
    for n_levels in (2, 3, 4, 5):
        for base in BASES:
            for vol_z in (zyx[0], 4096):
                chunks = [lv.chunks for lv in pyramid.fused_levels((vol_z,) + tuple(zyx[1:]), base, n_levels)]
                chunks = tuple(c for l, c in enumerate(chunks, start=1) if min(n >> l for n in zyx))
                if chunks and chunks not in seen:
                    seen.add(chunks)
                    out.append(list(chunks))
    return out


def block_volume(zyx, seed=0):
    rs = np.random.RandomState(sum(zyx) + seed)
    vol = rs.randint(0, 65536, zyx).astype(np.uint16)
    vol[: zyx[0] // 2, : zyx[1] // 2] |= 0xFFF0  # sums near 8 * 65535
    return vol


def source_bricks(vol, src_chunk, poison=False):
    """The block in the chunk order of an array with chunks ``src_chunk``; ``poison``: 0xFFFF wherever a brick sticks out
    of the block (what the store held there is nobody's business)."""
    bricks = fo.planes_to_bricks(vol, src_chunk)
    if poison:
        bricks[fo.planes_to_bricks(np.ones(vol.shape, np.uint8), src_chunk) == 0] = 0xFFFF
    return bricks


@pytest.mark.parametrize("zyx", BLOCKS)
def test_bricks_ref_equals_block_ref_and_never_reads_the_padding(zyx):
    vol = block_volume(zyx)
    sources = [(sc, source_bricks(vol, sc), source_bricks(vol, sc, poison=True)) for sc in SRC_CHUNKS]
    assert any((p != b).any() for _, b, p in sources)  # (there is padding to poison)
    for chunks in level_chunk_cases(zyx):
        want = engine.pyramid_block_ref(vol, chunks)
        for sc, bricks, poisoned in sources:
            for src in (bricks, poisoned):
                got = engine.pyramid_bricks_ref(src, zyx, sc, chunks)
                assert len(got) == len(want)
                for lvl, (g, w) in enumerate(zip(got, want), start=1):
                    assert g.shape == w.shape and g.tobytes() == w.tobytes(), (zyx, sc, chunks, lvl, src is poisoned)


@pytest.mark.parametrize("zyx", [(64, 36, 50), (7, 20, 44), (33, 10, 12), (5, 9, 11)])
@pytest.mark.parametrize("src_chunk", SRC_CHUNKS)
def test_bricks_ref_at_z_offsets_with_several_rows_and_a_second_block(zyx, src_chunk):
    rs = np.random.RandomState(5)
    vol = rs.randint(0, 65536, zyx).astype(np.uint16)
    chunks, z0s, rows = [(64, 16, 16), (40, 8, 8), (64, 3, 5)], [29, 3, 11], [2, 1, 1]
    got = engine.pyramid_bricks_ref(source_bricks(vol, src_chunk, True), zyx, src_chunk, chunks, z0s=z0s, rows=rows)
    want = engine.pyramid_block_ref(vol, chunks, z0s=z0s, rows=rows)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    # a second block into the same rows keeps the first block's planes
    vol2 = rs.randint(0, 65536, zyx).astype(np.uint16)
    z1s = [z + (zyx[0] >> l) for l, z in enumerate(z0s, start=1)]
    engine.pyramid_bricks_ref(source_bricks(vol2, src_chunk, True), zyx, src_chunk, chunks, z0s=z1s, bricks_out=got, rows=rows)
    engine.pyramid_block_ref(vol2, chunks, z0s=z1s, bricks=want, rows=rows)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert any(g.any() for g in got)


def test_bricks_ref_refusals():
    vol = np.zeros((16, 8, 8), np.uint16)
    with pytest.raises(ValueError):  # 8 planes from plane 2 need 3 rows of 4
        engine.pyramid_bricks_ref(source_bricks(vol, (4, 8, 8)), vol.shape, (4, 8, 8), [(4, 4, 4)], z0s=[2], rows=[2])
    with pytest.raises(ValueError):
        engine.pyramid_bricks_ref(source_bricks(vol, (4, 8, 8)).astype(np.float32), vol.shape, (4, 8, 8), [(4, 4, 4)])
    with pytest.raises(ValueError):  # not the bricks of this block
        engine.pyramid_bricks_ref(source_bricks(vol, (4, 8, 8)), vol.shape, (3, 8, 8), [(4, 4, 4)])


@pytest.mark.parametrize("Z,H,W,block_z,L,src_yx", [(150, 36, 50, 64, 3, (128, 128)), (131, 20, 44, 8, 4, (8, 8)),
                                                    (70, 10, 12, 16, 5, (5, 7))])  # fmt: skip
def test_levels_assembled_from_brick_blocks_equal_the_whole_volume_pyramid(Z, H, W, block_z, L, src_yx):
    rs = np.random.RandomState(Z)
    vol = rs.randint(0, 65536, (Z, H, W)).astype(np.uint16)
    levels = pyramid.fused_levels((Z, H, W), (1, 1, 64, 128, 128), L)
    whole = fo.pyramid(vol, L)
    src_chunk = (block_z,) + src_yx
    assert pyramid.pipelined_block_z(block_z, levels) == block_z
    rows = [-(-lv.shape[0] // lv.chunks[0]) for lv in levels]
    bricks = None
    for (z0, z1), shares in pyramid.fused_schedule(levels, 0, Z, block_z):
        z0s = [s.row * lv.chunks[0] + s.offset for s, lv in zip(shares, levels)]
        src = source_bricks(vol[z0:z1], src_chunk, poison=True)
        bricks = engine.pyramid_bricks_ref(src, (z1 - z0, H, W), src_chunk, [lv.chunks for lv in levels], z0s=z0s,
                                           bricks_out=bricks, rows=rows)  # fmt: skip
    for lv, b in zip(levels, bricks):
        assert np.array_equal(fo.bricks_to_planes(b, lv.shape), whole[lv.level]), lv


def test_pipelined_block_z_is_the_smallest_block_of_whole_source_chunks():
    L = pyramid.fused_levels
    for n_levels in (2, 3):
        assert pyramid.pipelined_block_z(64, L((4096, 2048, 2048), (1, 1, 64, 128, 128), n_levels)) == 64
    assert pyramid.pipelined_block_z(16, L((150, 203, 301), (16, 32, 32), 4)) == 16
    assert pyramid.pipelined_block_z(6, L((40, 64, 64), (6, 32, 32), 3)) == 12
    with pytest.raises(ValueError):
        pyramid.pipelined_block_z(3, L((150, 203, 301), (16, 32, 32), 4))
    for src_cz, levels in ((64, L((4096, 2048, 2048), (64, 128, 128), 3)), (6, L((40, 64, 64), (6, 32, 32), 3)),
                           (5, L((400, 64, 64), (40, 32, 32), 3))):  # fmt: skip
        bz = pyramid.pipelined_block_z(src_cz, levels)
        pyramid.fused_check_blocks(levels, bz)
        for smaller in range(src_cz, bz, src_cz):
            with pytest.raises(ValueError):
                pyramid.fused_check_blocks(levels, smaller)


def test_new_keywords_are_keyword_only_behind_the_references_parameters():
    checks = ((zd.compute_multiscale, {"pipelined": False, "device_codec": False, "device_decode": False, "io_threads": None}),
              (zd.destripe_zarr, {"pipelined_pyramid": False}), (zd.destripe_channel, {"pipelined_pyramid": False}))  # fmt: skip
    for fn, names in checks:
        params = inspect.signature(fn).parameters
        order = list(params)
        last_positional = max(i for i, n in enumerate(order) if params[n].kind is not inspect.Parameter.KEYWORD_ONLY)
        for n, default in names.items():
            assert params[n].kind is inspect.Parameter.KEYWORD_ONLY and order.index(n) > last_positional, (fn, n)
            assert params[n].default is default, (fn, n)
    sig = inspect.signature(pyramid.write_pyramid_levels).parameters
    assert [sig[n].default for n in ("pipelined", "device_codec", "device_decode", "io_threads")] == [False, False, False, None]
    assert isinstance(pyramid.LAST_PYRAMID, dict)


def _level0(tmp_path, dtype=np.uint16):
    p = str(tmp_path / "g" / "0")
    a = MiniZarrArray.create(p, (1, 1, 8, 16, 16), (1, 1, 2, 8, 8), dtype, compressor="blosc" if dtype == np.uint16 else None)
    a[0, 0] = np.arange(8 * 16 * 16).reshape(8, 16, 16).astype(dtype)
    return p, str(tmp_path / "g")


def test_refusals_that_precede_engine_creation(tmp_path):
    """Every one of these is a ``ValueError``; creating an engine without a GPU would be a ``DsxError``."""
    p, g = _level0(tmp_path)
    ms = lambda *a, **kw: zd.compute_multiscale(p, g, *a, 1, None, "t", n_levels=3, chunks=(1, 1, 2, 8, 8), **kw)  # noqa: E731
    for kw in ({"device_codec": True}, {"device_decode": True}, {"device_codec": "runs"}, {"device_decode": "any"},
               {"device_codec": 1}, {"device_decode": None}):  # fmt: skip
        with pytest.raises(ValueError, match="need pipelined=True"):  # the codec options without pipelined
            ms([2, 2, 2], **kw)
    with pytest.raises(ValueError, match="device_codec is False, True or"):
        ms([2, 2, 2], pipelined=True, device_codec="fast")
    with pytest.raises(ValueError, match="device_decode is False, True or"):
        ms([2, 2, 2], pipelined=True, device_decode="all")
    with pytest.raises(ValueError, match="only scale factors"):
        ms([2, 2, 4], pipelined=True)
    (tmp_path / "f").mkdir()
    pf, gf = _level0(tmp_path / "f", np.float32)
    with pytest.raises(ValueError, match="uint16"):
        zd.compute_multiscale(pf, gf, [2, 2, 2], 1, None, "t", n_levels=3, chunks=(1, 1, 2, 8, 8), pipelined=True)
    with pytest.raises(ValueError, match="Blosc uint16 input"):  # device_decode of a raw level 0
        raw = str(tmp_path / "raw" / "0")
        MiniZarrArray.create(raw, (1, 1, 8, 16, 16), (1, 1, 2, 8, 8), np.uint16, compressor=None)
        zd.compute_multiscale(raw, str(tmp_path / "raw"), [2, 2, 2], 1, None, "t", n_levels=3, chunks=(1, 1, 2, 8, 8),
                              pipelined=True, device_decode=True)  # fmt: skip
    with pytest.raises(ValueError, match="no z block"):  # source z chunk 3 under z chunks of 16
        odd = str(tmp_path / "odd" / "0")
        MiniZarrArray.create(odd, (1, 1, 150, 203, 301), (1, 1, 3, 32, 32), np.uint16, compressor=None)
        zd.compute_multiscale(odd, str(tmp_path / "odd"), [2, 2, 2], 1, None, "t", n_levels=4, chunks=(1, 1, 16, 32, 32),
                              compressor=None, pipelined=True)  # fmt: skip
    both = dict(fused_pyramid=True, pipelined_pyramid=True)
    with pytest.raises(ValueError, match="fused_pyramid and pipelined_pyramid"):
        zd.destripe_zarr(tmp_path / "x.zarr", "0", tmp_path / "o.zarr", (4, 16, 16), 0, 0, 1, None, tmp_path, tmp_path, None, {},
                         **both)  # fmt: skip
    with pytest.raises(ValueError, match="fused_pyramid and pipelined_pyramid"):
        zd.destripe_channel(tmp_path, tmp_path, "Ex_488_Em_525", tmp_path / "r", None, [], {}, {}, **both)
    assert not (tmp_path / "r").exists()  # (nothing was written)


class _HostBuffer:
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.mem = np.zeros(self.nbytes, np.uint8)
        self.ptr = self.mem.ctypes.data

    def array(self, shape, dtype, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.mem[offset : offset + n].view(dtype).reshape(shape)

    def free(self):
        pass


class _HostEngine(engine.DestripeEngine):
    """The engine calls of the pipelined pass with host memory for device memory and the host build for the kernel,
    every call synchronous: the pass's own logic (blocks, schedule, rows, chunk files) without a GPU.  The chunk I/O is
    the real one (``dsx_io_read_chunks`` / ``dsx_io_write_chunks`` take no context)."""

    def __init__(self, device=0):
        self._lib, self._ctx = engine.load_library(), None

    def close(self):
        pass

    def alloc(self, nbytes):
        return _HostBuffer(nbytes)

    alloc_host = alloc

    def copy_h2d_async(self, d_buf, host_array, stream=1, offset=0):
        d_buf.mem[offset : offset + host_array.nbytes] = host_array.reshape(-1).view(np.uint8)

    def copy_d2h_async(self, host_array, d_buf, stream=2, offset=0):
        host_array.reshape(-1).view(np.uint8)[:] = d_buf.mem[offset : offset + host_array.nbytes]

    def stream_wait(self, *a):
        pass

    event_record = event_sync = stream_wait

    def sync(self):
        pass

    def pyramid_bricks(self, d_src, zyx, src_chunk, chunks, d_bricks, z0s=None, zero=None, rows=None, d_work=None):
        src = d_src.mem[: engine.src_brick_elems(zyx, src_chunk) * 2].view(np.uint16)
        outs = []
        for lvl, (ck, b) in enumerate(zip(chunks, d_bricks), start=1):
            ny, nx = (-(-(n >> lvl) // c) if n >> lvl else 0 for n, c in zip(zyx[1:], ck[1:]))
            shape = (rows[lvl - 1], ny, nx) + tuple(ck)
            outs.append(b.mem[: int(np.prod(shape)) * 2].view(np.uint16).reshape(shape))
            if zero[lvl - 1] and zyx[0] >> lvl:
                outs[-1][:] = 0
        engine.pyramid_bricks_ref(src, zyx, src_chunk, chunks, z0s=z0s, bricks_out=outs, rows=rows)


@pytest.mark.parametrize("zyx,chunks,n_levels,compressor,block_z", [
    ((160, 200, 312), (1, 1, 64, 128, 128), 4, "blosc", 64),  # a row after two blocks, a 32-plane last block, clamped chunks
    ((150, 203, 301), (1, 1, 16, 32, 32), 4, None, 16),       # odd extents, ten blocks
    ((40, 64, 64), (1, 1, 6, 32, 32), 3, "zlib", 12),         # blocks of two source chunk rows
])  # fmt: skip
def test_the_pass_on_a_host_stand_in_for_the_device_writes_the_oracles_levels(tmp_path, monkeypatch, zyx, chunks, n_levels,
                                                                             compressor, block_z):  # fmt: skip
    vol = np.random.RandomState(1).randint(0, 65536, zyx).astype(np.uint16)
    g = str(tmp_path / "g")
    MiniZarrArray.create(g + "/0", (1, 1) + zyx, chunks, np.uint16, compressor=compressor)[0, 0] = vol
    monkeypatch.setattr(engine, "DestripeEngine", _HostEngine)
    shapes = zd.compute_multiscale(g + "/0", g, [2, 2, 2], 1, None, "t", n_levels=n_levels, chunks=chunks,
                                   compressor=compressor, pipelined=True, io_threads=4)  # fmt: skip
    want = fo.pyramid(vol, n_levels)
    assert shapes == [(1, 1) + w.shape for w in want[1:]]
    for lvl in range(1, n_levels):
        got = MiniZarrArray.open(g + "/" + str(lvl))
        assert got.matches((1, 1) + want[lvl].shape, tuple(min(c, n) for c, n in zip(chunks, (1, 1) + want[lvl].shape)),
                           np.uint16, compressor) and got.sep == "/"  # fmt: skip
        assert np.array_equal(got[0, 0], want[lvl]), lvl
        grid = [range(-(-n // c)) for n, c in zip(got.shape, got.chunks)]
        assert all(os.path.exists(got._chunk_path(i)) for i in itertools.product(*grid)), lvl  # written, not fill value
    assert not os.path.exists(g + "/" + str(n_levels))
    last = pyramid.LAST_PYRAMID
    n_chunks = int(np.prod([-(-n // c) for n, c in zip(zyx, chunks[-3:])]))
    assert last["route"] == "pipelined" and last["block_z"] == block_z and last["levels"] == list(range(1, n_levels))
    assert last["decode_routes"] == {"device": 0, "host": n_chunks, "fill": 0} and last["seconds"] > 0
