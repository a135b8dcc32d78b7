"""``k_zdec`` and ``k_zdec_all`` (``csrc/dsx_zdec_kernels.h``) held to what the kernels of the commit before the shared
match executor answered on an MI355X: the status of every task of ``tests/golden/zdec_task_statuses.npz`` and the
bytes of those that succeed, in one launch of 200 tasks; no byte outside a task's range changes."""

import pytest

import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu


def test_the_kernels_give_the_recorded_statuses_and_bytes():
    t = zc.status_table("device")
    e = eng_mod.DestripeEngine(0)
    try:
        out, status = zc.run_device(e, t)
    finally:
        e.close()
    zc.check(t, out, status, "dsx_blosc_decode_device")
