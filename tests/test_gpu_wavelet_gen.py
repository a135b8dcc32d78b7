"""The tap-count-generic wavelet kernels (``csrc/dsx_wavelet.h``: ``k_fwd_gen``, ``k_inv_gen``) on the device, over the
cases of ``tests/wavelet_gen_cases.py``: banks up to 104 taps (13 of the 105 banks need more than 64 KiB of dynamic LDS),
coefficient and result tiles that end on, one past and one short of a level, planes shorter than the filter.

Stage tests, one launch at a time, against the oracle's plain float64 ``dwt2`` / ``idwt2``:

(a) forward: level ``l`` of the engine against ``dwt2`` of the ENGINE's own ``aa_{l-1}`` (level 1: of float64
    ``log1p(x)``), so errors do not compound.  Bound: two passes of an ``F``-term FMA chain in float32,

        tol = 2.5 F 2^-24 |dec_lo|_1 |band|_1 max|input|      (+ 3 2^-24 |dec_lo|_1 |band|_1 max|log1p(x)| at level 1, logf)

    ``band = dec_lo`` for ``aa``, ``dec_hi`` (the column pass) for ``cH``.  A wrong tap, a patch origin off by one or a
    stale tile edge gives ``|tap| max|input|``: four or more orders above.
(b) fg/bg statistic and config choice, Otsu value and threshold per level: the bounds of ``test_stage_forward_and_
    thresholds``; an Otsu bin that differs goes through ``parity_util.find_otsu_ties``.
(c) synthesis, strict: float64 ``waverec2`` of the engine's OWN ``Delta_l`` (read back after the row filter), then
    ``(1 + x) exp(c0) + 1``: every pixel of the float32 result, no flip allowance -- the masks are the engine's own.
    Bound (``synthesis_reference``), per pixel: an FMA chain of ``n`` terms with float32 taps errs by at most
    ``2^-24 sum_j (n - j + 1) |term_j|`` (term ``j`` goes through the roundings of FMA ``j .. n - 1``, and its tap is
    rounded once).  Per level the row pass is a chain of ``F / 2`` terms (rec_lo on ``c_l`` and on ``Delta_l``) and the
    column pass one of ``F`` terms (rec_lo on the one, rec_hi on the other, interleaved); the error ``E_l`` of ``c_l``
    goes through both passes with absolute taps.  ``E_L = 0`` (``c_L = 0``), and

        relative tolerance of the result = 1.01 E_0 + 4 2^-24                      (expf, 1 + x, the final fmaf)

    asserted to stay below 1e-5 for every case.  The uint16 result is the float32 one clipped and truncated, exactly.

Then the whole path under the parity statement (d), the shading epilogue (e), the stack mode (f), the capacity limits
(g) and ``filter_streaks`` on its generic route with long banks (h).  The ``error / tol`` ratios of (a) and (c) are
printed per case; ``profiles/README.md`` records them."""

import ctypes
import warnings

import numpy as np
import pytest

import wavelet_gen_cases as wg
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import filtering, synth, wavelets
from oracle import destripe_oracle as orc
from parity_util import check_plane, find_otsu_ties, gpu_deltas, numerically_empty

pytestmark = pytest.mark.gpu

U = 2.0**-24  # unit round-off of float32
MAX_FLIPS = lambda size: max(3, int(2e-5 * size))  # noqa: E731  (as tests/test_gpu_parity.py)
CASES = wg.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


_RUNS = {}


def _run(engine, case):
    """One case through the engine with ``cells = nocells =`` its config, every stage read back; made once per case and
    shared by the stage tests (left unchanged by them)."""
    name, _, planes, _, _, _ = case
    if name in _RUNS:
        return _RUNS[name]
    n, h, w = planes.shape
    cfg = wg.config(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        engine.plan(h, w, cfg, cfg, wg.HIGH_INT, max_batch=n)
    r = {"levels": engine.levels, "shapes": [tuple(engine.level_shape(lv)) for lv in range(engine.levels)]}
    levels = range(engine.levels)
    try:
        engine.set_stop_after(1)
        engine.run(planes, out_dtype=np.float32)
        r["aa"] = [[engine.level_array(k, lv, eng_mod.STAGE_APPROX) for lv in levels] for k in range(n)]
        r["ch"] = [[engine.level_array(k, lv, eng_mod.STAGE_DETAIL) for lv in levels] for k in range(n)]
        r["stats"] = [engine.stats(k) for k in range(n)]
        r["thresholds"] = [[engine.thresholds(k, lv) for lv in levels] for k in range(n)]
        engine.set_stop_after(2)
        engine.run(planes, out_dtype=np.float32)
        r["delta"] = [[engine.level_array(k, lv, eng_mod.STAGE_DETAIL) for lv in levels] for k in range(n)]
    finally:
        engine.set_stop_after(0)
    r["out"], r["used"] = engine.run(planes, out_dtype=np.float32, return_cfg=True)
    r["out16"] = engine.run(planes, out_dtype=np.uint16)
    _RUNS[name] = r
    return r


def _l1(f):
    return float(np.abs(f).sum())


def forward_reference(bank, prev, first):
    """Float64 ``dwt2`` of ``prev`` and the bound (a) of the module docstring: ``(aa, cH, tol_aa, tol_cH)``."""
    aa, (ch, _, _) = orc.dwt2(prev, bank)
    F, lo, hi, top = len(bank[0]), _l1(bank[0]), _l1(bank[1]), float(np.abs(prev).max())
    tol = [2.5 * F * U * lo * band * top + (3 * U * lo * band * top if first else 0.0) for band in (lo, hi)]
    return aa, ch, tol[0], tol[1]


def synthesis_reference(bank, deltas, x):
    """Float64 result ``(1 + x) exp(c0) + 1`` of the Delta pyramid ``deltas`` (fine -> coarse) and the per-pixel relative
    tolerance (c) of the module docstring."""
    rec_lo, rec_hi = bank[2], bank[3]
    F = len(rec_lo)
    j = (F - 1 - np.arange(F)) // 2  # tap t is term j of its chain (synthesis convention of csrc/dsx_wavelet.h)
    alo, ahi = np.abs(rec_lo), np.abs(rec_hi)
    # roundings term j goes through (+ 1: its float32 tap): F / 2 - j of the row chain; in the column chain c's term is
    # FMA 2 j and Delta's FMA 2 j + 1 of F
    w_row, w_col_lo, w_col_hi = alo * (F // 2 - j + 1), alo * (F - 2 * j + 1), ahi * (F - 2 * j)
    none = np.zeros(F)
    c = np.zeros(deltas[-1].shape)
    err = np.zeros(deltas[-1].shape)
    for d in deltas[::-1]:
        d = d.astype(np.float64)
        c, err = c[: d.shape[0], : d.shape[1]], err[: d.shape[0], : d.shape[1]]  # waverec2's trim of the one-too-long level
        z = np.zeros(d.shape)
        a0 = orc.idwt_axis(c, z, rec_lo, none, 1)
        d0 = orc.idwt_axis(d, z, rec_lo, none, 1)
        err_a0 = orc.idwt_axis(err, z, alo, none, 1) + U * orc.idwt_axis(np.abs(c), z, w_row, none, 1)
        err_d0 = U * orc.idwt_axis(np.abs(d), z, w_row, none, 1)
        err = orc.idwt_axis(err_a0, err_d0, alo, ahi, 0) + U * orc.idwt_axis(np.abs(a0), np.abs(d0), w_col_lo, w_col_hi, 0)
        c = orc.idwt_axis(a0, d0, rec_lo, rec_hi, 0)
    hout, wout = x.shape[0] + x.shape[0] % 2, x.shape[1] + x.shape[1] % 2
    assert c.shape == (hout, wout)
    xp = np.pad(x.astype(np.float64), ((0, hout - x.shape[0]), (0, wout - x.shape[1])), mode="edge")
    return (1.0 + xp) * np.exp(c) + 1.0, 1.01 * err + 4 * U


def test_engine_level_shapes_follow_the_filter_length(engine):
    for case in CASES:
        r = _run(engine, case)
        assert r["shapes"] == wg.level_shapes(case[2].shape[1:], wg.taps(case[1]), r["levels"]), case[0]
        assert r["levels"] == (case[3] if case[3] is not None else r["levels"]) and r["levels"] >= 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_stage_level_by_level(engine, case):
    """(a): ``aa_l`` and ``cH_l`` of every level against float64 ``dwt2`` of the engine's own ``aa_{l-1}``."""
    name, wavelet, planes, _, _, _ = case
    bank = wg.bank_of(wavelet)
    r = _run(engine, case)
    worst, failed = 0.0, []
    for k in range(planes.shape[0]):
        prev = np.log1p(planes[k].astype(np.float64))
        for lv in range(r["levels"]):
            aa, ch, tol_aa, tol_ch = forward_reference(bank, prev, lv == 0)
            assert r["aa"][k][lv].shape == aa.shape and r["ch"][k][lv].shape == ch.shape
            for what, got, ref, tol in (("aa", r["aa"][k][lv], aa, tol_aa), ("cH", r["ch"][k][lv], ch, tol_ch)):
                ratio = float(np.abs(got - ref).max()) / tol
                worst = max(worst, ratio)
                if not ratio <= 1.0:  # (nan fails too)
                    bad = np.argwhere(~(np.abs(got - ref) <= tol))
                    failed.append((k, lv, what, ratio, len(bad), bad[:4].tolist()))
            prev = r["aa"][k][lv].astype(np.float64)
    print("[wavelet_gen] forward {}: worst error / tol {:.3f}".format(name, worst))
    assert not failed, (name, failed)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_statistic_config_otsu_and_thresholds(engine, case):
    """(b): the statistic fused into the level-1 kernel, the config it selects, Otsu value and threshold per level."""
    name, _, planes, _, _, _ = case
    ocfg = wg.config(case, oracle=True)
    r = _run(engine, case)
    for k in range(planes.shape[0]):
        which, fore, back = orc.select_config(planes[k].astype(np.float64), ocfg, ocfg, wg.HIGH_INT)
        f, b, c = r["stats"][k]
        assert c == which == int(r["used"][k]), (name, k)
        assert abs(f - fore) <= 1e-9 * max(1.0, abs(fore)) and abs(b - back) <= 1e-9 * max(1.0, abs(back)), (name, k)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, stages = orc.log_space_fft_filtering(planes[k], return_stages=True, **ocfg)
            stages = stages[::-1]
            assert len(stages) == r["levels"]
            ties = find_otsu_ties([t[0] for t in r["thresholds"][k]], stages, r["ch"][k])
            if ties is not None:
                print("[wavelet_gen] {} plane {}: Otsu tie at level index {}".format(
                    name, k, [lv for lv, t in enumerate(ties) if t is not None]))
                _, stages = orc.log_space_fft_filtering(planes[k], return_stages=True, otsu_overrides=ties[::-1], **ocfg)
                stages = stages[::-1]
        for lv, st in enumerate(stages):
            if numerically_empty(st, lv):
                continue
            otsu, thr = r["thresholds"][k][lv]
            assert abs(thr - st["threshold"]) <= 2e-5 * max(st["threshold"], 1e-3), (name, k, lv, thr, st["threshold"])
            assert abs(otsu - st["otsu"]) <= 1e-4 * max(st["otsu"], 1e-6), (name, k, lv, otsu, st["otsu"])
    if name.startswith("batch"):
        assert set(int(u) for u in r["used"]) == {0, 1}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_synthesis_stage_strict(engine, case):
    """(c): every pixel of the float32 result against float64 ``waverec2`` of the engine's own Delta pyramid; the uint16
    result is the float32 one clipped to [0, 65535] and truncated."""
    name, wavelet, planes, _, _, _ = case
    bank = wg.bank_of(wavelet)
    r = _run(engine, case)
    worst, top_tol, failed = 0.0, 0.0, []
    for k in range(planes.shape[0]):
        ref, tol = synthesis_reference(bank, r["delta"][k], planes[k])
        assert r["out"][k].shape == ref.shape
        top_tol = max(top_tol, float(tol.max()))
        rel = np.abs(r["out"][k].astype(np.float64) - ref) / np.abs(ref)
        ratio = float((rel / tol).max())
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad = np.argwhere(~(rel <= tol))
            failed.append((k, ratio, float(rel.max()), len(bad), bad[:4].tolist()))
        want16 = np.clip(r["out"][k], 0.0, 65535.0).astype(np.uint16)
        np.testing.assert_array_equal(r["out16"][k], want16, err_msg="%s plane %d: uint16 cast" % (name, k))
    print("[wavelet_gen] synthesis {}: worst error / tol {:.3f} (largest relative tol {:.2e})".format(name, worst, top_tol))
    assert top_tol < 1e-5, (name, top_tol)
    assert not failed, (name, failed)
    if name == "saturate":
        assert float(r["out"].max()) > 65535.0 and int(r["out16"].max()) == 65535


def _whole_path(engine, case, max_batch=None):
    """(d) for every plane of a case: ``gpu_deltas`` + ``check_plane`` with the config pair of ``wg.configs``; a uint16
    plane must satisfy the statement against the reference's float64 regime or its float32 regime (the two differ from
    each other at Otsu plateaus; the engine computes in float32), the float64 one is tried first."""
    name, _, planes, _, _, _ = case
    cells, nocells = wg.configs(case)
    ocells, onocells = wg.configs(case, oracle=True)
    n = planes.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        deltas = gpu_deltas(engine, planes, high_int=wg.HIGH_INT, max_batch=max_batch or n, cells=cells, nocells=nocells)
        out, used = engine.run(planes, out_dtype=np.float32, return_cfg=True)
        for k in range(n):
            err = None
            for regime in (np.float32,) if planes.dtype == np.float32 else (np.uint16, np.float32):
                img = planes[k].astype(regime)
                which, _, _ = orc.select_config(img, onocells, ocells, wg.HIGH_INT)
                assert int(used[k]) == which, (name, k)
                try:
                    check_plane(out[k].astype(np.float64), img, deltas[k], (name, k, np.dtype(regime).name),
                                ocells if which else onocells, MAX_FLIPS)  # fmt: skip
                    err = None
                    break
                except AssertionError as e:
                    err = e
            if err is not None:
                raise err
    return out, used


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_whole_path_parity(engine, case):
    out, used = _whole_path(engine, case)
    if case[0].startswith("batch"):
        assert set(int(u) for u in used) == {0, 1}
        # cohorts of two planes: bit-identical to the single cohort
        cells, nocells = wg.configs(case)
        engine.plan(case[2].shape[1], case[2].shape[2], cells, nocells, wg.HIGH_INT, max_batch=2)
        out2, used2 = engine.run(case[2], out_dtype=np.float32, return_cfg=True)
        np.testing.assert_array_equal(used2, used)
        assert np.array_equal(out2, out)


def test_shading_epilogue_on_an_odd_plane_with_a_larger_dark_plane():
    """(e): ``k_inv_gen``'s flatfield epilogue with db33: the result of a 97 x 131 plane is 98 x 132, so is the flat; the
    dark plane is two rows and three columns larger and is indexed with its own pitch."""
    name = "db33"
    bank = wavelets.filter_bank(name)
    cells = {"wavelet": name, "level": 1, "sigma": 32, "max_threshold": 3}
    nocells = {"wavelet": name, "level": 1, "sigma": 64, "max_threshold": 12}
    x = synth.synthetic_plane(3, 97, 131)
    rng = np.random.RandomState(7)
    flat = (0.8 + 0.4 * rng.rand(98, 132)).astype(np.float32)
    dark = (90 + 20 * rng.rand(100, 135)).astype(np.float32)
    sc = {"retrospective": True, "flatfield": flat, "darkfield": dark, "tile_config": {}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = filtering.filter_stripes(x, "X_0_Y_0", nocells, cells, sc, wg.HIGH_INT)
        ref = orc.filter_stripes(x, "X_0_Y_0", dict(nocells, wavelet=bank), dict(cells, wavelet=bank), sc, wg.HIGH_INT)
    assert got.dtype == np.uint16 and got.shape == ref.shape == (98, 132)
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("name,level", [("db33", 1), ("sym4", 2)])
def test_stack_mode_with_a_bank(engine, name, level):
    """(f): ``GenFwdArgs::shared`` -- the planes of a stack share one min / max of cH^2, so one Otsu threshold, per
    level.  A stack of tests/golden/stack3d.npz (5 x 64 x 96, one plane with a bright block)."""
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack3d.npz")) as g:
        stack = g["a__in"]
    bank = wavelets.filter_bank(name)
    cfg = {"wavelet": name, "level": level, "sigma": 64, "max_threshold": 12}
    ocfg = dict(cfg, wavelet=bank)
    n = stack.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # the oracle's stack mode, stage by stage (destripe_oracle._log_space_fft_filtering_stack with the stages kept)
        per_plane = [orc.wavedec2(np.log1p(p.astype(np.float64)), level=level, bank=bank) for p in stack]
        width_fraction = cfg["sigma"] / min(stack.shape[1:])
        stages = []  # coarse -> fine
        for i in range(1, level + 1):
            ch = np.stack([c[i][0] for c in per_plane])
            orc.filter_level(ch, ch.shape[1] * width_fraction, cfg["max_threshold"], stages)
        stages = stages[::-1]
        ref = orc.log_space_fft_filtering(stack, **ocfg)
        alone = np.stack([orc.log_space_fft_filtering(p, **ocfg) for p in stack])
        assert np.abs(alone - ref).max() / np.abs(ref).max() > 1e-3  # the shared threshold matters on this stack
        engine.set_stack_mode(True)
        try:
            deltas = gpu_deltas(engine, stack, high_int=wg.HIGH_INT, max_batch=n, cells=cfg, nocells=cfg)
            thr = [[engine.thresholds(k, lv) for lv in range(engine.levels)] for k in range(n)]
            out = engine.run(stack, out_dtype=np.float32)
        finally:
            engine.set_stack_mode(False)
        out_alone = engine.run(stack, out_dtype=np.float32)
        assert engine.levels == level
        for k in range(n):
            assert thr[k] == thr[0], (name, k, thr[k], thr[0])
            for lv, st in enumerate(stages):
                otsu, t = thr[k][lv]
                assert abs(t - st["threshold"]) <= 2e-5 * max(st["threshold"], 1e-3), (name, lv, t, st["threshold"])
                assert abs(otsu - st["otsu"]) <= 1e-4 * max(st["otsu"], 1e-6), (name, lv, otsu, st["otsu"])
            # per-plane view of the stack's stages; the Otsu value is the stack's, so the per-plane tie analysis is off
            st_k = [dict(st, ch=st["ch"][k], ch_filtered=st["ch_filtered"][k]) for st in stages]
            deltas[k].otsu = None
            check_plane(out[k].astype(np.float64), stack[k], deltas[k], (name, "stack", k), ocfg, MAX_FLIPS, ref=ref[k], stages=st_k)
        assert np.abs(out_alone.astype(np.float64) - out).max() / np.abs(out).max() > 1e-3


def test_capacity_limits(engine):
    """(g): 104 taps are taken (case ``capacity``), 106 are refused by the Python layer and by the C ABI, and the
    context is usable afterwards."""
    too_long = wg.padded_bank("coif17", pad=2)
    assert len(too_long.dec_lo) == 106
    with pytest.raises(ValueError, match="106 taps"):
        wavelets.filter_bank(too_long)
    dp = ctypes.POINTER(ctypes.c_double)
    filters = [np.ascontiguousarray(getattr(too_long, f)) for f in ("dec_lo", "dec_hi", "rec_lo", "rec_hi")]
    rc = engine._lib.dsx_set_wavelet(engine._ctx, *[f.ctypes.data_as(dp) for f in filters], 106)
    assert rc == -5 and eng_mod._ERRORS[rc] == "DSX_ELIMIT"
    case = ("after_elimit", "sym4", synth.synthetic_plane(1, 58, 121)[None], 2, 64, 4)
    _whole_path(engine, case)


@pytest.mark.parametrize("name", ["db33", "coif17"])
def test_filter_streaks_generic_route_with_long_banks(name):
    """(h): ``csrc/dsx_streaks.h`` carries its own ``lo[kMaxTaps]``; the dual-band filter on its generic route."""
    from tests import streaks_oracle as so
    from tests.test_gpu_streaks import _within

    img = synth.synthetic_plane(4, 150, 201)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = filtering.filter_streaks(img, sigma=(16, 32), level=1, wavelet=name)
        _, ref = so.filter_streaks(img, (16, 32), level=1, wavelet=name)
    assert out.dtype == np.float64 and out.shape == img.shape
    _within(out, ref)
