"""The native finish of a flat on the host (``dsx_gauss_smooth_f64_ref`` / ``dsx_flat_finish_ref``, ``csrc/dsx_smooth.h``)
against today's NumPy finish: the smoothing inside a bound derived from the two orders of summation, SciPy's golden
planes, the fill, the crop, the routes of ``estimate_fields(finish=...)``, argument errors, and the same code built with
g++ from ``tests/host/flat_finish_check.cpp`` under ASan / UBSan as its own process.  No GPU needed."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import flat_finish_cases as fc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import flatfield_estimation as fe

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "flat_estimation.npz"))
DSX_EINVAL, DSX_EVALUE = -1, -8
U = 2.0**-53


# ---- taps and cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", fc.SIGMAS + (0.124, 0.125, 7.3, 63.9))
def test_gauss_taps_are_the_taps_of_gaussian_smooth(sigma):
    r, t = eng_mod.gauss_taps(sigma)
    assert t.dtype == np.float64 and t.shape == (r + 1,)
    if sigma == 0:
        assert r == 0 and t[0] == 1.0
        return
    assert r == int(4.0 * sigma + 0.5) <= eng_mod.GAUSS_MAX_RADIUS
    x = np.arange(-r, r + 1, dtype=np.float64)
    full = np.exp(-0.5 / (sigma * sigma) * x * x)
    full /= full.sum()
    assert np.array_equal(full, full[::-1])  # exactly symmetric: the right half says it all
    assert np.array_equal(t, full[r:])


def test_the_cases_cover_what_they_claim():
    cases = fc.smooth_cases()
    shapes = {c.plane.shape for c in cases}
    assert {c.sigma for c in cases} == set(map(float, fc.SIGMAS))
    for axis, name in ((0, "y"), (1, "x")):
        sizes = {s[axis] for s in shapes}
        for tile in fc.TILES[name]:
            assert {tile - 1, tile, tile + 1, 2 * tile + 1} <= sizes, (name, tile)
        for sigma in (2, 2.25, 32, 64):
            r = fc.radius(sigma)
            assert {r, r + 1, 2 * r + 1} <= sizes, (name, sigma)
    assert {(1, 1), (1, 37), (37, 1), (2, 3), (3, 5)} <= shapes
    assert any(c.plane.shape[1] % 2 == 1 and c.plane.shape[1] > 64 for c in cases)
    assert any(c.lead for c in cases) and any(not c.lead for c in cases)
    assert any((c.plane < 0).any() for c in cases) and any((c.plane >= 0).all() and (c.plane % 1 == 0).all() for c in cases)
    assert max(c.plane.size for c in cases) <= 300 * 520
    by = {c.name: c for c in fc.finish_cases()}
    c = by["even_count_half"]
    assert np.median(c.rank[0][c.valid > 0]) == 12.0 and (c.valid > 0).sum() == 4
    c = by["high_values"]
    assert c.rank.max() >= 16384 and c.rank[0].min() < 65535
    assert by["large_nq2"].shape[0] * by["large_nq2"].shape[1] > 512 * 256 > fc.MEAN_LANES


# ---- the two passes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.smooth_cases(), ids=fc.smooth_ids())
def test_host_smooth_is_gaussian_smooth_within_the_derived_bound(case):
    """One pass errs by at most (2r + 2) u sum(t |a|) in either order of summation, so the two orders differ by at most
    8 (r + 1) u G(|a|) to first order over both passes; 9 (r + 1) u G(|a|) is asked."""
    before = case.plane.copy()
    got = fc.smooth_reference()[case.name]
    want = fe.gaussian_smooth(case.plane, case.sigma)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(case.plane, before)
    r = fc.radius(case.sigma)
    bound = 9.0 * (r + 1) * U * fe.gaussian_smooth(np.abs(case.plane), case.sigma)
    err = np.abs(got - want)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(case.name, "largest error / bound:", worst)
    assert np.all(err <= bound)
    if case.sigma == 0:
        assert np.array_equal(got, case.plane)


@pytest.mark.parametrize("i", range(5))
def test_host_smooth_is_scipy_gaussian_filter(i):
    plane, sigma, ref = GOLDEN["plane_{}".format(i)], float(GOLDEN["sigma_{}".format(i)]), GOLDEN["smooth_{}".format(i)]
    got = eng_mod.gauss_smooth_ref(plane, eng_mod.gauss_taps(sigma)[1])
    err = np.abs(got - ref).max()
    print("case", i, "max abs error", err, "relative", err / np.abs(ref).max())
    assert err <= 1e-12 * np.abs(ref).max()


def test_contract_in_numpy_is_the_host_build_bit_for_bit():
    """The contract written out with exact rational arithmetic per fused multiply-add (fractions) on a tiny plane."""
    from fractions import Fraction

    rs = np.random.RandomState(3)
    a = rs.standard_normal((3, 4)) * 100.0
    r, t = eng_mod.gauss_taps(1)

    def fold(j, n):
        j %= 2 * n
        return j if j < n else 2 * n - 1 - j

    def line(v):
        out = []
        for i in range(len(v)):
            acc = float(t[0]) * float(v[i])
            for k in range(1, r + 1):
                s = float(v[fold(i - k, len(v))]) + float(v[fold(i + k, len(v))])
                acc = float(Fraction(float(t[k])) * Fraction(s) + Fraction(acc))  # one rounding: a fused multiply-add
            out.append(acc)
        return out

    tmp = np.array([line(a[:, x]) for x in range(a.shape[1])]).T
    want = np.array([line(tmp[y]) for y in range(a.shape[0])])
    assert np.array_equal(eng_mod.gauss_smooth_ref(a, t), want)


# ---- the finish ------------------------------------------------------------------------------------------------------------
def _adjacent(a, b):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.mark.parametrize("case", fc.finish_cases(), ids=fc.finish_ids())
def test_host_finish_is_the_numpy_finish_within_a_float32_spacing(case):
    flat, dark = fc.finish_reference()[case.name]
    want_flat, want_dark = fc.numpy_finish(case)
    assert flat.dtype == np.float32 and flat.shape == case.shape
    print(case.name, "flats that differ:", int((flat != want_flat).sum()), "of", flat.size)
    assert _adjacent(flat, want_flat)
    assert (dark is None) == (case.rank.shape[0] == 1)
    if dark is not None:
        assert dark.dtype == np.float32 and dark.shape == case.shape
        assert _adjacent(dark, want_dark)
    assert flat.min() >= np.float32(case.floor)


def test_the_fill_is_the_median_of_the_seen_pixels():
    taps = eng_mod.gauss_taps(0)[1]  # no smoothing: dark is the filled plane itself
    rank = np.array([[[10, 13, 500, 20, 700, 11]]], np.uint16).repeat(2, axis=0)
    valid = np.array([[1, 1, 0, 1, 0, 1]], np.uint16)
    flat, dark = eng_mod.flat_finish_ref(rank, valid, (1, 6), taps, 0.1)
    assert dark.tolist() == [[10.0, 13.0, 12.0, 20.0, 12.0, 11.0]]  # (11 + 13) / 2
    assert np.array_equal(flat, (dark.astype(np.float64) / (78.0 / 6.0)).astype(np.float32))
    valid[0, 3] = 0  # three seen: 10, 11, 13
    assert eng_mod.flat_finish_ref(rank, valid, (1, 6), taps, 0.1)[1].tolist() == [[10.0, 13.0, 11.0, 11.0, 11.0, 11.0]]
    rank[:, 0, :2] = (11, 14)  # four seen again, 11, 11, 14 and ... no: 11, 14, 11 -> three; make it even
    valid[0, 3] = 1  # 11, 14, 20, 11 -> (11 + 14) / 2 = 12.5
    assert eng_mod.flat_finish_ref(rank, valid, (1, 6), taps, 0.1)[1].tolist() == [[11.0, 14.0, 12.5, 20.0, 12.5, 11.0]]
    # an unseen region takes the median of the rest
    rs = np.random.RandomState(5)
    rank = rs.randint(0, 65536, (1, 20, 30)).astype(np.uint16)
    valid = np.ones((20, 30), np.uint16)
    valid[5:15, 10:20] = 0
    dark = eng_mod.flat_finish_ref(np.concatenate([rank, rank]), valid, (20, 30), taps, 0.1)[1]
    assert np.all(dark[5:15, 10:20] == np.float32(np.median(rank[0][valid > 0])))
    assert np.array_equal(dark[valid > 0], rank[0][valid > 0].astype(np.float32))


def test_a_stored_plane_larger_than_the_image_is_cropped():
    rs = np.random.RandomState(6)
    rank = rs.randint(100, 5000, (2, 32, 48)).astype(np.uint16)
    valid = rs.randint(0, 3, (32, 48)).astype(np.uint16)
    taps = eng_mod.gauss_taps(1.5)[1]
    want = eng_mod.flat_finish_ref(rank[:, :31, :47], valid[:31, :47], (31, 47), taps, 0.2)
    rank[:, 31, :], rank[:, :, 47], valid[31, :], valid[:, 47] = 65535, 65535, 3, 3
    got = eng_mod.flat_finish_ref(rank, valid, (31, 47), taps, 0.2)
    assert got[0].shape == (31, 47) and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_an_unseen_image_raises_the_existing_error():
    rank = np.full((1, 4, 6), 9, np.uint16)
    valid = np.zeros((4, 6), np.uint16)
    valid[3, :] = 1  # seen only outside the image
    with pytest.raises(eng_mod.NoSeenPixel):
        eng_mod.flat_finish_ref(rank, valid, (3, 6), [1.0], 0.1)
    lib = eng_mod.load_library()
    flat = np.full((3, 6), 7, np.float32)
    vp = ctypes.c_void_p
    rc = lib.dsx_flat_finish_ref(rank.ctypes.data_as(vp), valid.ctypes.data_as(vp), 4, 6, 3, 6, 1, (ctypes.c_double * 1)(1.0), 0,
                                 0.1, flat.ctypes.data_as(vp), None)  # fmt: skip
    assert rc == DSX_EVALUE and np.all(flat == 7)
    stack = np.full((3, 4, 6), 50, np.uint16)
    for finish in fe.FINISH_ROUTES:
        with pytest.raises(ValueError) as err:
            fe.estimate_fields(stack, valid_range=(100, 200), finish=finish)
        assert str(err.value) == "estimate_fields: no pixel has a value inside valid_range (100, 200)"


# ---- estimate_fields(finish=...) on host stacks ------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(smoothing=3.0), dict(smoothing=32.0, dark_quantile=0.05, valid_range=(300, 3500)),
                                     dict(smoothing=0, dark_quantile=0.25, floor=0.95)], ids=["flat", "dark_window", "sigma0"])  # fmt: skip
def test_estimate_fields_native_on_a_host_stack(options):
    rs = np.random.RandomState(9)
    y, x = np.mgrid[0:41, 0:53]
    shade = 1.0 - 0.4 * (((y - 20) / 20.0) ** 2 + ((x - 26) / 26.0) ** 2)
    stack = np.clip(rs.randint(200, 4000, (9, 41, 53)) * shade, 0, 65535).astype(np.uint16)
    numpy_fields = fe.estimate_fields(stack, **options)
    assert fe.LAST_FIELDS["finish"] == "numpy" and sorted(fe.LAST_FIELDS["seconds"]) == ["finish", "rank"]
    again = fe.estimate_fields(stack, finish="numpy", **options)
    native = fe.estimate_fields(stack, finish="native", **options)
    assert fe.LAST_FIELDS["finish"] == "native" and all(v >= 0 for v in fe.LAST_FIELDS["seconds"].values())
    assert sorted(native) == ["baseline", "darkfield", "flatfield", "valid"]
    assert again["flatfield"].tobytes() == numpy_fields["flatfield"].tobytes()
    assert np.array_equal(native["valid"], numpy_fields["valid"])
    assert native["flatfield"].dtype == np.float32 and native["flatfield"].shape == (41, 53)
    assert _adjacent(native["flatfield"], numpy_fields["flatfield"])
    if "dark_quantile" in options:
        assert _adjacent(native["darkfield"], numpy_fields["darkfield"])
    else:
        assert native["darkfield"] is None
    assert native["baseline"].shape == (9,) and not native["baseline"].any()


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_option_errors_come_before_any_library_call(monkeypatch):
    stack = np.full((2, 4, 4), 100, np.uint16)

    def no_call(*a, **k):
        raise AssertionError("a library call was made")

    for name in ("stack_rank_ref", "flat_finish_ref", "gauss_smooth_ref", "load_library", "DestripeEngine"):
        monkeypatch.setattr(eng_mod, name, no_call)
    for bad in ("gpu", "NATIVE", "", None, 1, b"native"):
        with pytest.raises(ValueError):
            fe.estimate_fields(stack, finish=bad)
    with pytest.raises(ValueError):
        fe.estimate_fields(stack, finish="native", smoothing=64.5)
    with pytest.raises(ValueError):
        fe.shading_correction(list(stack), {"finish": "gpu"})
    with pytest.raises(ValueError):
        fe.slide_flat_estimation({"ch": {}}, "ch", [0], {"finish": "native", "smoothing": 65}, None, None)
    with pytest.raises(ValueError):
        fe.estimate_channel_flats("nowhere", "ch", {"0": []}, {}, "out", finish="gpu")
    with pytest.raises(TypeError):
        fe.estimate_fields(stack, finished="native")
    assert "finish" in fe.ESTIMATOR_OPTIONS
    for sigma in (64.5, -1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError):
            eng_mod.gauss_taps(sigma)


def test_numpy_finish_still_takes_any_sigma():
    stack = np.random.RandomState(1).randint(100, 200, (3, 6, 7)).astype(np.uint16)
    assert fe.estimate_fields(stack, smoothing=80.0)["flatfield"].shape == (6, 7)


def test_c_abi_argument_rules():
    lib = eng_mod.load_library()
    vp, f64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    tmp, out = np.full((3, 4), 7.0), np.full((3, 4), 7.0)
    taps = np.array([0.5, 0.25])

    def smooth(in_=a, H=3, W=4, t=taps, r=1, tmp_=tmp, out_=out):
        p = lambda x: None if x is None else x.ctypes.data_as(vp)  # noqa: E731
        return lib.dsx_gauss_smooth_f64_ref(p(in_), H, W, None if t is None else t.ctypes.data_as(f64p), r, p(tmp_), p(out_))

    for bad in (dict(in_=None), dict(t=None), dict(tmp_=None), dict(out_=None), dict(H=0), dict(W=0), dict(H=-3), dict(r=-1),
                dict(r=257), dict(H=1 << 16, W=1 << 15), dict(tmp_=a), dict(tmp_=out)):  # fmt: skip
        assert smooth(**bad) == DSX_EINVAL, bad
    assert np.all(out == 7.0) and np.all(tmp == 7.0)  # nothing was written
    assert smooth() == 0 and not np.all(out == 7.0)
    inplace = a.copy()
    assert smooth(in_=inplace, out_=inplace) == 0 and np.array_equal(inplace, out)  # d_out == d_in is allowed

    rank = np.full((2, 4, 6), 9, np.uint16)
    valid = np.ones((4, 6), np.uint16)
    flat, dark = np.full((3, 5), 7, np.float32), np.full((3, 5), 7, np.float32)

    def finish(rank_=rank, valid_=valid, Hs=4, Ws=6, H=3, W=5, n_q=2, t=taps, r=1, floor=0.1, flat_=flat, dark_=dark):
        p = lambda x: None if x is None else x.ctypes.data_as(vp)  # noqa: E731
        return lib.dsx_flat_finish_ref(p(rank_), p(valid_), Hs, Ws, H, W, n_q, None if t is None else t.ctypes.data_as(f64p), r,
                                       floor, p(flat_), p(dark_))  # fmt: skip

    for bad in (dict(rank_=None), dict(valid_=None), dict(t=None), dict(flat_=None), dict(dark_=None), dict(n_q=0), dict(n_q=3),
                dict(H=5), dict(W=7), dict(H=0), dict(W=0), dict(r=-1), dict(r=257), dict(floor=0.0), dict(floor=-1.0),
                dict(floor=float("nan")), dict(floor=float("inf")), dict(Hs=1 << 16, Ws=1 << 15)):  # fmt: skip
        assert finish(**bad) == DSX_EINVAL, bad
    assert np.all(flat == 7) and np.all(dark == 7)
    assert finish(n_q=1, dark_=None) == 0 and np.all(dark == 7) and not np.all(flat == 7)  # no dark asked: not touched
    assert finish() == 0

    n = ctypes.c_size_t()
    assert lib.dsx_flat_finish_work_bytes(3, 5, ctypes.byref(n)) == 0 and n.value >= 2 * 8 * 15 + 4 * 65536 + 8 * 4096
    assert lib.dsx_flat_finish_work_bytes(0, 5, ctypes.byref(n)) == DSX_EINVAL
    assert lib.dsx_flat_finish_work_bytes(1 << 16, 1 << 15, ctypes.byref(n)) == DSX_EINVAL
    assert lib.dsx_flat_finish_work_bytes(3, 5, None) == DSX_EINVAL
    assert eng_mod.flat_finish_work_bytes((3, 5)) == lib.dsx_flat_finish_work_bytes(3, 5, ctypes.byref(n)) + n.value

    # the Python wrappers refuse before the library is asked; there the radius is len(taps) - 1, and a radius that is
    # given and says otherwise is refused
    for kwargs in (dict(taps=np.ones(258)), dict(radius=1), dict(taps=[0.5, 0.25], radius=0), dict(radius=True), dict(taps=np.ones((2, 2))), dict(taps=[]), dict(taps=[np.nan]), dict(shape=(3,)),
                   dict(shape=(0, 4)), dict(shape=(3.0, 4))):  # fmt: skip
        with pytest.raises(ValueError):
            eng_mod.smooth_args(**dict(dict(shape=(3, 4), taps=[1.0]), **kwargs))
    for kwargs in (dict(stored_shape=(2, 6)), dict(n_q=3), dict(n_q=True), dict(floor=0), dict(floor="1"), dict(stored_shape=(4,))):
        with pytest.raises(ValueError):
            eng_mod.flat_finish_args(**dict(dict(stored_shape=(4, 6), shape=(3, 5), n_q=2, taps=[1.0], floor=0.1), **kwargs))
    with pytest.raises(ValueError):
        eng_mod.gauss_smooth_ref(a.astype(np.float32), taps)
    with pytest.raises(ValueError):
        eng_mod.gauss_smooth_ref(a, taps, radius=2)
    with pytest.raises(ValueError):
        eng_mod.flat_finish_ref(rank, valid, (3, 5), taps, 0.1, radius=0)
    assert np.array_equal(eng_mod.gauss_smooth_ref(a, taps, radius=1), eng_mod.gauss_smooth_ref(a, taps))
    with pytest.raises(ValueError):
        eng_mod.flat_finish_ref(rank, valid[:3], (3, 5), taps, 0.1)


# ---- the host build as a program of its own, under sanitizers ------------------------------------------------------------------
def test_host_build_under_sanitizers(tmp_path):
    """tests/host/flat_finish_check.cpp with ASan / UBSan: the results, no access outside the planes, and the launch
    geometry of every case shape over every radius (the program returns 4 when a tile would not cover or fit)."""
    exe = str(tmp_path / "flat_finish_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "host", "flat_finish_check.cpp")], check=True)  # fmt: skip
    picked = [c for c in fc.smooth_cases() if c.plane.size <= 45 * 131]
    assert len(picked) >= 30
    for i, c in enumerate(picked):
        H, W = c.plane.shape
        r, taps = eng_mod.gauss_taps(c.sigma)
        raw, tap_file, res = str(tmp_path / "plane.raw"), str(tmp_path / "taps.raw"), str(tmp_path / "smooth.out")
        c.plane.tofile(raw)
        taps.tofile(tap_file)
        run = subprocess.run([exe, "smooth", raw, str(H), str(W), tap_file, str(r), str(i & 1), res], capture_output=True, text=True)
        assert run.returncode == 0, (c.name, run.returncode, run.stderr[-2000:])
        assert np.array_equal(np.fromfile(res, np.float64).reshape(H, W), fc.smooth_reference()[c.name]), c.name
    for c in fc.finish_cases():
        if c.shape[0] * c.shape[1] > 45 * 131:
            continue
        (n_q, Hs, Ws), (H, W) = c.rank.shape, c.shape
        r, taps = eng_mod.gauss_taps(c.sigma)
        files = [str(tmp_path / n) for n in ("rank.raw", "valid.raw", "taps.raw", "finish.out")]
        c.rank.tofile(files[0]), c.valid.tofile(files[1]), taps.tofile(files[2])
        args = [exe, "finish", files[0], files[1], Hs, Ws, H, W, n_q, files[2], r, repr(c.floor), files[3]]
        run = subprocess.run([str(a) for a in args], capture_output=True, text=True)
        assert run.returncode == 0, (c.name, run.returncode, run.stderr[-2000:])
        got = np.fromfile(files[3], np.float32).reshape(n_q, H, W)
        flat, dark = fc.finish_reference()[c.name]
        assert got[0].tobytes() == flat.tobytes(), c.name
        assert n_q == 1 or got[1].tobytes() == dark.tobytes(), c.name
    np.zeros((1, 2, 2), np.uint16).tofile(files[0]), np.zeros((2, 2), np.uint16).tofile(files[1]), np.ones(1).tofile(files[2])
    run = subprocess.run([exe, "finish", files[0], files[1], "2", "2", "2", "2", "1", files[2], "0", "0.1", files[3]])
    assert run.returncode == 6  # no pixel seen
