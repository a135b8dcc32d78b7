"""The launch chain on the CPU: what csrc/dsx_chain.h decides (which kernels, grids, blocks, LDS sizes) for every case of
tools/chain_trace.py's table against the launches recorded from a kernel trace on the MI355X
(tests/golden/chain_launches.json, written by ``tools/chain_trace.py golden`` from the trace of the commit BEFORE the chain
was split into stages, with the CU count of that machine), and the rules the kernels rely on over the value lists of
tools/fuzz_parity.py's switch table.  Built with g++ from tests/host/dsx_host_check.cpp; no GPU needed."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import chain_trace  # noqa: E402

GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "chain_launches.json")))
SRC = os.path.join(REPO, "tests", "host", "dsx_host_check.cpp")


def _build(path, sanitize):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", path, SRC], check=True)
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("chain") / "dsx_host_check"), False)


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("chain_san") / "dsx_host_check"), True)


def _chain(exe, case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSX_")}
    env.update({k: str(v) for k, v in case["env"].items()})
    r = subprocess.run([exe, "chain"] + chain_trace.host_check_args(case, GOLDEN["cus"]), env=env, check=True,
                       capture_output=True, text=True)  # fmt: skip
    return json.loads(r.stdout)


def test_the_table_is_the_recorded_one():
    assert [c["name"] for c in chain_trace.CASES] == list(GOLDEN["launches"])
    assert GOLDEN["cus"] > 0


@pytest.mark.parametrize("case", chain_trace.CASES, ids=[c["name"] for c in chain_trace.CASES])
def test_launches_are_the_recorded_ones(exe, case):
    """Kernel name with template arguments, grid and block of every launch, in enqueue order.  (The trace's LDS column
    carries the kernels' static LDS only, so the dynamic LDS bytes are held to what the kernels index instead: the
    twiddle table and one row buffer per wave of the RECORDED block size.)"""
    got = _chain(exe, case)
    want = GOLDEN["launches"][case["name"]]
    assert [g[:3] for g in got] == [w[:3] for w in want]
    F = int(dict(kv.split("=") for kv in chain_trace.host_check_args(case, 0))["flen"])
    for name, _, block, lds, M in got:
        if name.startswith("k_rowfilter_wide"):
            assert lds == 8 * M
        elif name.startswith(("k_rowfilter", "k_rowfinal")):
            assert lds == 8 * M * (block // 64 + 1) <= 160 * 1024
        elif name.startswith("k_fwd_gen"):  # the (32 + F - 2) x (64 + F - 2) patch, odd pitch, and the two column-pass tiles
            assert lds == 4 * ((32 + F - 2) + 32) * (64 + F - 2 + 1)
        elif name.startswith("k_inv_gen"):
            assert lds == 4 * 2 * (16 + F // 2 - 1) * ((32 + F // 2 - 1) + 1 + 64 + 1)
        else:
            assert lds == 0


def test_geometry_rules(exe):
    """nseg / rows_per_seg cover the rows exactly once, the fused final kernel's segments start at even rows, k_hist's
    16-bit counters cannot carry, the row filters' LDS fits 160 KiB for every forced DSX_ROW_WPB, a k_rowfinal plan id
    is the classifier's, blk_end of the merged coarse launch increases up to the grid (dsx_host_check chain-rules)."""
    r = json.loads(subprocess.run([exe, "chain-rules"], check=True, capture_output=True, text=True).stdout)
    assert r["ok"] and r["checked"] > 1_000_000, r


def test_chain_mode_is_clean_under_asan_and_ubsan(exe, exe_sanitized):
    for case in chain_trace.CASES:
        assert _chain(exe_sanitized, case) == _chain(exe, case)
