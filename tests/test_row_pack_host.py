"""The host decisions of the packed coarse row filter (k_rowfilter_pack) on the CPU: tests/host/row_pack_check.cpp holds
csrc/dsx_chain.h's virtual-butterfly map, pack factor and launch geometry for the six transform lengths of the coarse
levels of a 2048^2 plane and 1 ... 4 row pairs per wave.  Built with g++, plain and with the host sanitizers; no GPU."""

import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "row_pack_check.cpp")


def _run(tmp_path, sanitize):
    exe = str(tmp_path / "row_pack_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSX_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_row_pack_decisions(tmp_path, sanitize):
    """Every virtual butterfly index of a wave maps to one butterfly of one live pair and they are all reached, with fewer
    live pairs than the pack factor too; the pack factor is the one of least modelled cost within the register and the
    LDS bound (3 at M = 260, 4 at 132, 144, 36, 20, 12: the model table of DESIGN.md 4.3b); the blocks of a launch
    cover every pair of every level once and their LDS stays within 160 KiB."""
    r = _run(tmp_path, sanitize)
    assert r["ok"] and r["failed"] == 0 and r["checked"] > 100_000, r
    assert r["pack"] == [3, 4, 4, 4, 4, 4]
