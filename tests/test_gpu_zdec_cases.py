"""``k_zdec`` (``csrc/dsx_zdec_kernels.h``) held to bytes that no decoder of this project made: the tables of
tests/zdec_cases.py, which tests/test_zdec_cases_host.py runs through the host build, here through the kernel.  The
kernel's driver (``zstd_wave``, ``lz_wave``, the wave copies and un-shuffles) exists only on the device; these tests are
what holds it to libzstd's input on every zstd mode, at every task layout, and to the host build's status words on
malformed zstd frames (each of which went through the CPU sanitizer builds in the host file first)."""

import time

import numpy as np
import pytest

import test_zstd_decoder_host as zh
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod
from test_gpu_device_decode import _device_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    return zc.mode_frames()


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _launch(engine, table, who):
    """One launch of the table on the device: checked against the expectations, then against the host build as a whole."""
    t0 = time.perf_counter()
    out, st = zc.run_device(engine, table)
    print("{}: {} tasks, launch {:.3f} s, with copies {:.3f} s".format(who, len(table.rows), zc.LAUNCH_SECONDS[-1][1],
                                                                     time.perf_counter() - t0))  # fmt: skip
    zc.check(table, out, st, who)
    ref, ref_st = zc.run_ref(table)
    assert np.array_equal(st, ref_st), (who, [(table.names[i], int(st[i]), int(ref_st[i]))
                                              for i in np.flatnonzero(st != ref_st)[:8]])  # fmt: skip
    return out, st, ref


def test_mode_frames_decode_to_what_libzstd_was_given(engine, frames, tmp_path):
    """Section A: every frame a bare zstd task, one launch per flag; then the proof, over the frames the kernel
    decoded, that they asked for every path of its driver."""
    decoded = set(range(len(frames)))
    for flag in zc.FLAGS:
        out, st, ref = _launch(engine, zc.mode_table(frames, flag), "A, flag {:#x}".format(flag))
        assert np.array_equal(out, ref)  # (every task succeeds: no unspecified byte)
        decoded &= set(np.flatnonzero(st == 0).tolist())
    decoded = [frames[i] for i in sorted(decoded)]
    exe = zc.build_check_exe(str(tmp_path / "zstd_dec_check"))
    cov = zc.coverage(decoded, zc.frame_stats(exe, tmp_path, decoded))
    assert not zc.missing_cases(cov), zc.missing_cases(cov)


def test_blosc_level_frames(engine, tmp_path):
    """c-blosc's three block sizes at every zstd level through the frame reader: the tasks a run launches."""
    cases = zc.blosc_level_frames()
    paths = []
    for i, (name, frame, raw) in enumerate(cases):
        paths.append(str(tmp_path / "c{:02d}".format(i)))
        with open(paths[-1], "wb") as f:
            f.write(frame)
    cb = len(cases[0][2])
    packed, tasks, _ = eng_mod.io_read_frames(paths, cb)
    t0 = time.perf_counter()
    dev, st = _device_decode(engine, packed, tasks, cb * len(cases))
    print("Blosc level: {} tasks, {:.3f} s with copies".format(len(tasks), time.perf_counter() - t0))
    ref, ref_st = eng_mod.blosc_decode_ref(packed, tasks, cb * len(cases))
    assert not st.any() and not ref_st.any()
    for i, (name, _, raw) in enumerate(cases):
        assert dev[i * cb : (i + 1) * cb].tobytes() == raw, name
    assert np.array_equal(dev, ref)


def test_layout_sweep(engine):
    """Section B: every kind, flag and split form at every length and residue, one launch, canaries between."""
    t, facts = zc.layout_table()
    assert not [k for k, v in zc.layout_paths(facts).items() if v == 0]
    out, st, ref = _launch(engine, t, "B")
    assert np.array_equal(out, ref)


def test_malformed_tasks_between_good_ones(engine, frames):
    """Section C: the host build's status words (the documented ones where ``_broken_frames`` has one), exact good
    neighbours, no byte outside any task's range."""
    t = zc.malformed_table(zc.good_neighbours(frames))
    documented = {k: v[2] for k, v in zh._broken_frames().items()}
    out, st, _ = _launch(engine, t, "C")
    for name, want in documented.items():
        assert int(st[t.names.index(name)]) == want, name
