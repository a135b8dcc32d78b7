"""``run_task_host`` (``csrc/dsx_zdec_task.h``) held to the record of the three chained runners it replaced: the status
of every task of ``tests/golden/zdec_task_statuses.npz`` and the bytes of those that succeed, through
``dsx_blosc_decode_ref`` and through the stand-alone g++ build.  No GPU needed."""

import struct
import subprocess

import numpy as np

import zdec_cases as zc


def test_the_table_covers_the_task_model():
    t = zc.status_table("host")
    words = {r[4] for r in t.rows}
    assert {k | f for k in range(8) for f in (0, 0x100, 0x200, 0x400, 0x300, 0x600, 0x500, 0x800)} <= words
    assert all(sum(1 for r in t.rows if r[4] == w and r[3] == 32) == 3 for w in words)  # valid, cut, raw
    assert sorted(r[4] & 0xFF for r in t.rows if r[3] == 31) == list(range(8))
    assert len(t.rows) == 200 and {0, 1, 4, 12} <= set(t.status)


def test_the_host_runner_gives_the_recorded_statuses_and_bytes():
    t = zc.status_table("host")
    out, status = zc.run_ref(t)
    zc.check(t, out, status, "dsx_blosc_decode_ref")


def test_the_gxx_build_gives_the_recorded_statuses_and_bytes(tmp_path_factory, tmp_path):
    t = zc.status_table("host")
    exe = zc.build_task_exe(tmp_path_factory)
    rec, res = str(tmp_path / "rec.bin"), str(tmp_path / "out.bin")
    zc.write_records(rec, [(bytes(t.packed[r[0] : r[0] + r[2]]), r[3], r[4]) for r in t.rows if r[4] & 0xFF])
    subprocess.run([exe, "decode", rec, res], check=True)
    blob, at = open(res, "rb").read(), 0
    for i, r in enumerate(t.rows):
        if not r[4] & 0xFF:
            continue  # (a fill task has its value where a record has its offset)
        st = struct.unpack("<i", blob[at : at + 4])[0]
        at += 4
        assert st == t.status[i], (t.names[i], st, t.status[i])
        if st == 0:
            assert blob[at : at + r[3]] == t.expect[i], t.names[i]
            at += r[3]
    assert at == len(blob)


def test_host_and_device_records_agree():
    """The kernels and the host runner of the recorded commit answered every task of the table alike."""
    rec = np.load(zc.STATUS_TABLE)
    assert np.array_equal(rec["host_status"], rec["device_status"]) and np.array_equal(rec["host_out"], rec["device_out"])
