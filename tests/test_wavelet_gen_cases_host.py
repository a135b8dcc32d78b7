"""The case list of the generic wavelet kernels (``tests/wavelet_gen_cases.py``) on the CPU: every case runs through the
oracle in both regimes, every bank of the list is a perfect-reconstruction bank (the padded 104-tap one included), the
tile residues are what the list promises, and the dynamic-LDS sizes of ``csrc/dsx_chain.h`` (``dsx_host_check genlds``)
stay within ``kLdsLimit`` with the 64 KiB crossover between 64 and 66 taps.  No GPU needed."""

import json
import os
import subprocess
import warnings

import numpy as np
import pytest

import wavelet_gen_cases as wg
from oracle import destripe_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "dsx_host_check.cpp")
CASES = wg.cases()
IDS = [c[0] for c in CASES]


def test_the_list_is_fixed_and_holds_what_it_promises():
    again = wg.cases()
    assert [c[0] for c in again] == IDS and len(set(IDS)) == len(IDS)
    for a, b in zip(CASES, again):
        assert a[3:] == b[3:] and a[2].dtype == b[2].dtype and np.array_equal(a[2], b[2])
    F = {c[0]: wg.taps(c[1]) for c in CASES}
    assert (F["lds_under"], F["lds_over"], F["longest"], F["capacity"]) == (64, 66, 102, 104)
    assert (F["short"], F["deep"], F["bior39"], F["rbio39"], F["tile_edges_db38_on"], F["tile_edges_sym4_on"]) == (2, 32, 20, 20, 76, 8)
    assert F["capacity"] == wg.wavelets.MAX_TAPS
    assert wg.gen_fwd_lds_bytes(F["lds_under"]) <= wg.LDS_DEFAULT < wg.gen_fwd_lds_bytes(F["lds_over"])
    assert {c[2].dtype for c in CASES} == {np.dtype(np.uint16), np.dtype(np.float32)}
    for c in CASES:
        assert max(c[2].shape[1:]) <= wg.MAX_PLANE and "rbio3.1" != c[1]
    # biorthogonal: rec is not the reversed dec, and the L1 norms differ
    for name in ("bior3.9", "rbio3.9"):
        dec_lo, dec_hi, rec_lo, _ = wg.bank_of(name)
        assert not np.allclose(rec_lo, dec_lo[::-1]) and abs(np.abs(dec_lo).sum() - np.abs(dec_hi).sum()) > 0.1
    # both configs are chosen in the batch, and some result of `saturate` leaves the uint16 range
    batch = CASES[IDS.index("batch_u16")]
    assert [orc.select_config(p, None, None, wg.HIGH_INT)[0] for p in batch[2]] == [1, 0, 0, 0, 1]
    assert CASES[IDS.index("saturate")][2].max() > 65535


def test_tile_residues():
    assert wg.tile_residues() == {"db38": [(0, 0, 0, 0), (1, 1, 1, 1), (15, 31, 31, 63)],
                                  "sym4": [(0, 0, 0, 0), (1, 1, 1, 1), (15, 31, 31, 63)]}  # fmt: skip
    for c in CASES:
        if c[0].startswith("tile_edges"):
            assert c[3] == 2  # the level-2 synthesis writes c_1 of the level-1 shape in tiles of 32 x 64


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_runs_both_regimes_and_the_bank_reconstructs(case):
    name, wavelet, planes, level, sigma, max_threshold = case
    bank = wg.bank_of(wavelet)
    F = len(bank[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "level too high": the wrap cases, as pywt warns in the reference
        x = planes[0]
        outs = []
        for regime in (np.uint16, np.float32) if x.dtype == np.uint16 else (np.float32, np.float64):
            out, stages = orc.log_space_fft_filtering(x.astype(regime), return_stages=True, **wg.config(case, oracle=True))
            assert out.shape == (x.shape[0] + x.shape[0] % 2, x.shape[1] + x.shape[1] % 2) and np.isfinite(out).all()
            assert len(stages) >= 1
            assert [s["ch"].shape for s in stages[::-1]] == wg.level_shapes(x.shape, F, len(stages)), name
            if level is not None:
                assert len(stages) == level
            outs.append(out)
        # the reference's own two regimes agree far inside the parity statement, apart from threshold decisions
        assert np.median(np.abs(outs[0] - outs[1]) / np.abs(outs[0])) < 5e-6
        # float64 round trip of the bank at the case's depth, cut to the plane
        logx = np.log1p(x.astype(np.float64))
        back = orc.waverec2(orc.wavedec2(logx, level=len(stages), bank=bank), bank)
        assert np.abs(back[: x.shape[0], : x.shape[1]] - logx).max() <= 1e-12, name
    if name == "short":
        assert [s["ch"].shape for s in stages] == [(2, 3), (3, 5), (5, 9), (9, 17), (17, 33)]
    if name == "deep":
        assert len(stages) == 3
    if name == "wrap_coif17":
        assert [s["ch"].shape for s in stages] == [(81, 83), (62, 65)]


def test_gen_lds_sizes_of_the_chain_header(tmp_path):
    """``gen_fwd_lds_bytes`` / ``gen_inv_lds_bytes`` as the launches take them (tests/host/dsx_host_check.cpp includes
    csrc/dsx_chain.h itself): the closed forms, all within ``kLdsLimit``, 64 KiB crossed between 64 and 66 taps."""
    exe = str(tmp_path / "dsx_host_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-o", exe, SRC], check=True)
    r = json.loads(subprocess.run([exe, "genlds"], check=True, capture_output=True, text=True).stdout)
    assert r["limit"] == 160 * 1024
    assert sorted(int(k) for k in r["taps"]) == list(range(2, 105, 2))
    for k, (fwd, inv) in r["taps"].items():
        F = int(k)
        assert fwd == wg.gen_fwd_lds_bytes(F) == 4 * ((30 + F) + 32) * (63 + F)
        assert inv == 4 * 2 * (15 + F // 2) * ((31 + F // 2) + 1 + 64 + 1)
        assert 0 < inv <= fwd <= r["limit"], (F, fwd, inv)
    assert r["taps"]["64"][0] == 64008 <= wg.LDS_DEFAULT < r["taps"]["66"][0] == 66048
    assert r["taps"]["102"][0] == 108240
    over = [n for n in wg.wavelets.wavelist() if n != "dmey" and wg.gen_fwd_lds_bytes(wg.taps(n)) > wg.LDS_DEFAULT]
    assert len(over) == 13 and {"db33", "db38", "coif11", "coif17"} <= set(over)
