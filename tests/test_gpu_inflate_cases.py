"""``k_zdec_all`` (``csrc/dsx_zdec_kernels.h``: ``inflate_wave``, ``lz_wave``) held to the tables of
tests/inflate_cases.py, which tests/test_inflate_decoder_host.py runs through the host build and the sanitizer
builds: the kernel returns the bytes that were encoded, the status words of the host build, and changes no byte
outside a task's destination."""

import time

import numpy as np
import pytest

import inflate_cases as ic
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu
E = eng_mod


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _launch(engine, table, who):
    """One launch of the table on the device: checked against the expectations, then against the host build."""
    t0 = time.perf_counter()
    out, st = zc.run_device(engine, table)
    print("{}: {} tasks, launch {:.3f} s, with copies {:.3f} s".format(who, len(table.rows), zc.LAUNCH_SECONDS[-1][1],
                                                                     time.perf_counter() - t0))  # fmt: skip
    zc.check(table, out, st, who)
    ref, ref_st = zc.run_ref(table)
    assert np.array_equal(st, ref_st), (who, [(table.names[i], int(st[i]), int(ref_st[i]))
                                              for i in np.flatnonzero(st != ref_st)[:8]])  # fmt: skip
    return out, st, ref


def test_zlib_streams(engine):
    """The corpus of Python's zlib and the hand-assembled streams, plain and under both un-shuffles."""
    streams = ic.zlib_corpus() + ic.hand_streams()
    for flag in zc.FLAGS:
        out, st, ref = _launch(engine, ic.zlib_table(streams, flag), "zlib corpus, flag {:#x}".format(flag))
        assert not st.any() and np.array_equal(out, ref)


def test_blosclz_corner_cases(engine):
    t = zc.Table()
    for i, (name, z, data) in enumerate(ic.blosclz_hand_streams()):
        t.add(name, z, len(data), E.TASK_BLOSCLZ, data, dst_res=i % 16, src_res=i % 4)
    out, st, ref = _launch(engine, t, "blosclz corners")
    assert not st.any() and np.array_equal(out, ref)


def test_layout_sweep(engine):
    """Table B for the new kinds: tasks of 0 .. 70 001 bytes, every flag and split form, every residue."""
    t, _ = ic.layout_table()
    out, st, ref = _launch(engine, t, "B (zlib, blosclz)")
    assert not st.any() and np.array_equal(out, ref)


def test_one_256_kib_block_per_codec(engine):
    out, st, ref = _launch(engine, ic.big_block_table(), "256 KiB blocks")
    assert not st.any() and np.array_equal(out, ref)


def test_malformed_streams_between_good_ones(engine):
    """The status words of the host build, exact good neighbours, no byte outside any task's range."""
    t = ic.malformed_table()
    good = ic.blosclz_hand_streams()[0]
    for name, z, n, st in ic.blosclz_malformed():
        t.add("good blosclz", good[1], len(good[2]), E.TASK_BLOSCLZ, good[2])
        t.add(name, z, n, E.TASK_BLOSCLZ, None, status=st)
    out, st, _ = _launch(engine, t, "malformed")
    for i, name in enumerate(t.names):
        assert (int(st[i]) == 0) == name.startswith("good"), (name, int(st[i]))


def test_mixed_table_of_old_and_new_kinds(engine):
    """Tasks of both kernels in one table: each is decoded once, by its own kernel."""
    t = zc.Table()
    raw = zc._payload(30000)
    for i in range(3):
        t.add("zstd", zc._code(E.TASK_ZSTD, raw), len(raw), E.TASK_ZSTD, raw)
        t.add("zlib", ic.code(E.TASK_ZLIB, raw), len(raw), E.TASK_ZLIB, raw)
        t.add("lz4", zc._code(E.TASK_LZ4, raw), len(raw), E.TASK_LZ4, raw)
        t.add("blosclz", ic.code(E.TASK_BLOSCLZ, raw), len(raw), E.TASK_BLOSCLZ, raw)
        t.add("stored", raw, len(raw), E.TASK_STORED, raw)
        t.add("fill", b"", 100, E.TASK_FILL, b"\x34\x12" * 50, fill=0x1234)
        t.add("kind 7", raw[:50], 50, 7, None, status=4)
    out, st, ref = _launch(engine, t, "mixed kinds")
