"""The native finish of a flat on the device (``csrc/dsx_smooth.h``: ``DestripeEngine.gauss_smooth`` /
``DestripeEngine.flat_finish``) against its host build, bit for bit, on every case of ``flat_finish_cases.py``; then
``finish="native"`` through ``estimate_channel_flats``, ``slide_flat_estimation`` and ``shading_correction`` on the small
channel of ``test_gpu_flat_estimation.py``, and ``finish="numpy"`` unchanged."""

import ctypes
import os

import numpy as np
import pytest

import flat_finish_cases as fc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import filtering, mini_tiff, synth
from aind_smartspim_destripe_amd import flatfield_estimation as fe
from aind_smartspim_destripe_amd import zarr_destriper as zd
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray

pytestmark = pytest.mark.gpu

DSX_EINVAL = -1
GUARD = -12345.678


@pytest.fixture(scope="module")
def eng():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


# ---- the two passes ------------------------------------------------------------------------------------------------------
def _guarded(e, elems, lead, fill=None):
    """A device buffer for ``elems`` float64 that start ``2 + lead`` elements in (16-byte aligned for ``lead == 0``, only
    8-byte aligned for ``lead == 1``), every element set to GUARD; returns ``(buffer, address of the plane)``."""
    d = e.alloc(8 * (elems + 4))
    host = np.full(elems + 4, GUARD)
    if fill is not None:
        host[2 + lead : 2 + lead + elems] = fill.reshape(-1)
    d.upload(host)
    return d, d.ptr + 8 * (2 + lead)


def _plane_of(d, elems, lead):
    host = d.download(elems + 4, np.float64)
    assert np.all(host[: 2 + lead] == GUARD) and np.all(host[2 + lead + elems :] == GUARD)
    return host[2 + lead : 2 + lead + elems]


@pytest.mark.parametrize("case", fc.smooth_cases(), ids=fc.smooth_ids())
def test_device_smooth_is_the_host_build(eng, case):
    H, W = case.plane.shape
    _, taps = eng_mod.gauss_taps(case.sigma)
    want = fc.smooth_reference()[case.name]
    d_in, p_in = _guarded(eng, H * W, case.lead, case.plane)
    d_tmp, p_tmp = _guarded(eng, H * W, case.lead)
    d_out, p_out = _guarded(eng, H * W, case.lead)
    try:
        eng.gauss_smooth(p_in, (H, W), taps, d_tmp=p_tmp, d_out=p_out)
        eng.sync()
        got = _plane_of(d_out, H * W, case.lead).reshape(H, W)
        assert np.array_equal(_plane_of(d_in, H * W, case.lead).reshape(H, W), case.plane)
        _plane_of(d_tmp, H * W, case.lead)
        assert got.tobytes() == want.tobytes()
        eng.gauss_smooth(p_in, (H, W), taps, d_tmp=p_tmp, d_out=p_in)  # d_out == d_in
        eng.sync()
        assert _plane_of(d_in, H * W, case.lead).reshape(H, W).tobytes() == want.tobytes()
    finally:
        for d in (d_in, d_tmp, d_out):
            d.free()


def test_device_smooth_allocates_what_is_not_given(eng):
    case = fc.smooth_cases()[-3]
    d_in = eng.alloc(case.plane.nbytes)
    d_in.upload(case.plane)
    d_out, d_tmp = eng.gauss_smooth(d_in, case.plane.shape, eng_mod.gauss_taps(case.sigma)[1])
    try:
        eng.sync()
        assert d_out.download(case.plane.shape, np.float64).tobytes() == fc.smooth_reference()[case.name].tobytes()
    finally:
        for d in (d_in, d_out, d_tmp):
            d.free()


# ---- the finish ------------------------------------------------------------------------------------------------------------
def _device_finish(e, rank, valid, shape, taps, floor):
    n_q, (H, W) = rank.shape[0], shape
    d_rank, d_valid = e.alloc(max(rank.nbytes, 16)), e.alloc(max(valid.nbytes, 16))
    d_flat, d_dark = e.alloc(4 * (H * W + 2)), e.alloc(4 * (H * W + 2))
    try:
        d_rank.upload(rank)
        d_valid.upload(valid)
        for d in (d_flat, d_dark):
            d.upload(np.full(H * W + 2, -7.0, np.float32))
        e.flat_finish(d_rank, d_valid, rank.shape[1:], shape, n_q, taps, floor, d_flat=d_flat.ptr + 4, d_dark=d_dark.ptr + 4)
        flat, dark = d_flat.download(H * W + 2, np.float32), d_dark.download(H * W + 2, np.float32)
        assert flat[0] == -7.0 and flat[-1] == -7.0 and dark[0] == -7.0 and dark[-1] == -7.0
        if n_q == 1:
            assert np.all(dark == -7.0)
        assert np.array_equal(d_rank.download(rank.shape, np.uint16), rank)
        assert np.array_equal(d_valid.download(valid.shape, np.uint16), valid)
        return flat[1:-1].reshape(H, W), dark[1:-1].reshape(H, W) if n_q == 2 else None
    finally:
        for d in (d_rank, d_valid, d_flat, d_dark):
            d.free()


@pytest.mark.parametrize("case", fc.finish_cases(), ids=fc.finish_ids())
def test_device_finish_is_the_host_build(eng, case):
    want_flat, want_dark = fc.finish_reference()[case.name]
    flat, dark = _device_finish(eng, case.rank, case.valid, case.shape, eng_mod.gauss_taps(case.sigma)[1], case.floor)
    assert flat.tobytes() == want_flat.tobytes()
    assert (dark is None) == (want_dark is None)
    if dark is not None:
        assert dark.tobytes() == want_dark.tobytes()
        flat1, none = _device_finish(eng, case.rank[:1], case.valid, case.shape, eng_mod.gauss_taps(case.sigma)[1], case.floor)
        assert none is None and flat1.tobytes() == want_flat.tobytes()  # n_q = 1 of the same planes


def test_device_finish_argument_and_value_errors(eng):
    rank = np.full((1, 4, 6), 9, np.uint16)
    valid = np.zeros((4, 6), np.uint16)
    valid[3, :] = 1  # seen only outside the image
    with pytest.raises(eng_mod.NoSeenPixel):
        _device_finish(eng, rank, valid, (3, 6), [1.0], 0.1)
    valid[:] = 1
    flat, _ = _device_finish(eng, rank, valid, (3, 6), [1.0], 0.1)  # the context goes on after the refusal
    assert np.all(flat == 1.0)
    d = eng.alloc(4096)
    vp, f64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    taps = (ctypes.c_double * 2)(0.5, 0.25)
    lib, ctx = eng._lib, eng._ctx
    try:
        d.upload(np.zeros(512, np.float64))
        p = vp(d.ptr)
        q, w = vp(d.ptr + 1024), vp(d.ptr + 2048)
        calls = [lambda: lib.dsx_gauss_smooth_f64_device(ctx, None, 3, 4, taps, 1, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, None, 1, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, taps, 1, None, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, taps, 1, q, None),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, taps, 1, p, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 0, 4, taps, 1, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, taps, 257, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 3, 4, taps, -1, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(ctx, p, 1 << 16, 1 << 15, taps, 1, q, w),
                 lambda: lib.dsx_gauss_smooth_f64_device(None, p, 3, 4, taps, 1, q, w),
                 lambda: lib.dsx_flat_finish_device(ctx, None, p, 4, 6, 3, 5, 1, taps, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, None, 4, 6, 3, 5, 1, taps, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 1, None, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 1, taps, 1, 0.1, None, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 2, taps, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 1, taps, 1, 0.1, q, None, None),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 5, 5, 1, taps, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 3, taps, 1, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 1, taps, 257, 0.1, q, None, w),
                 lambda: lib.dsx_flat_finish_device(ctx, p, p, 4, 6, 3, 5, 1, taps, 1, 0.0, q, None, w)]  # fmt: skip
        for i, call in enumerate(calls):
            assert call() == DSX_EINVAL, i
        eng.sync()
        assert not d.download(512, np.float64).any()  # nothing was launched
        for kwargs in (dict(taps=np.ones(258)), dict(shape=(0, 4)), dict(shape=(1 << 16, 1 << 15)), dict(radius=3)):
            with pytest.raises(ValueError):
                eng.gauss_smooth(d, **dict(dict(shape=(3, 4), taps=[1.0]), **kwargs))
    finally:
        d.free()


# ---- the option through the estimators --------------------------------------------------------------------------------------
CHANNEL = "Ex_488_Em_525"
PARAMS = {"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG}
NAMES = ["431040_368180", "431040_394100", "457080_368180", "457080_394100"]
SIDES = {"0": NAMES[:2], "1": NAMES[2:]}
OPTIONS = dict(smoothing=2.0, dark_quantile=0.05)


def _vignette(H, W):
    y = (np.arange(H) - (H - 1) / 2) / ((H - 1) / 2)
    x = (np.arange(W) - (W - 1) / 2) / ((W - 1) / 2)
    return 1.0 - 0.25 * (y[:, None] ** 2 + x[None, :] ** 2)


def _channel(root, sides, Z=16, H=32, W=48):
    vols = {}
    for names in sides.values():
        for name in names:
            a = MiniZarrArray.create(str(root / "data" / CHANNEL / (name + ".zarr") / "0"), (1, 1, Z, H, W), (1, 1, 8, 16, 16),
                                     np.uint16, compressor="zlib")  # fmt: skip
            vol = synth.synthetic_stack(Z, H, W, n_unique=8).astype(np.float64) * (4.0 + NAMES.index(name)) * _vignette(H, W)[None]
            vols[name] = np.clip(vol, 0, 65535).astype(np.uint16)
            a[0, 0] = vols[name]
    return vols


def _host_stack(vols, names, zs):
    H, W = vols[names[0]].shape[1:]
    tiles = [filtering.destripe_planes(vols[name][zs], name, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG, None, 2700,
                                       out_dtype=np.uint16) for name in names]  # fmt: skip
    return np.ascontiguousarray(np.concatenate(tiles)[:, :H, :W])


def _adjacent(a, b):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.fixture(scope="module")
def channel(tmp_path_factory):
    root = tmp_path_factory.mktemp("flat_finish_channel")
    vols = _channel(root, SIDES)
    native = fe.estimate_channel_flats(root / "data", CHANNEL, SIDES, PARAMS, root / "flats_native", plane_step=4, finish="native",
                                       **OPTIONS)  # fmt: skip
    last_native = dict(fe.LAST_ESTIMATE)
    numpy_paths = fe.estimate_channel_flats(root / "data", CHANNEL, SIDES, PARAMS, root / "flats_numpy", plane_step=4,
                                            finish="numpy", **OPTIONS)  # fmt: skip
    last_numpy = dict(fe.LAST_ESTIMATE)
    default = fe.estimate_channel_flats(root / "data", CHANNEL, SIDES, PARAMS, root / "flats_default", plane_step=4, **OPTIONS)
    return root, vols, native, numpy_paths, default, last_native, last_numpy


def test_native_channel_flats_equal_the_host_builds_bit_for_bit(channel):
    root, vols, native, numpy_paths, default, _, _ = channel
    zs = fe.sampled_planes(16, 8, 1, 4)
    for side, p_native, p_numpy, p_default in zip(("0", "1"), native, numpy_paths, default):
        assert os.path.basename(p_native) == "estimated_flat_laser_{}_{}.tif".format(CHANNEL, side)
        stack = _host_stack(vols, SIDES[side], zs)
        got = mini_tiff.imread(p_native)
        assert got.dtype == np.float32 and got.shape == (32, 48)
        assert got.tobytes() == fe.estimate_fields(stack, finish="native", **OPTIONS)["flatfield"].tobytes()
        today = fe.estimate_fields(stack, **OPTIONS)["flatfield"]
        assert _adjacent(got, today)
        # finish="numpy" on the device, asked for or by default: today's result
        assert mini_tiff.imread(p_numpy).tobytes() == today.tobytes()
        assert mini_tiff.imread(p_default).tobytes() == today.tobytes()


def test_the_record_names_the_route_and_its_seconds(channel):
    *_, last_native, last_numpy = channel
    for last, route in ((last_native, "native"), (last_numpy, "numpy")):
        assert last["finish"]["route"] == route
        assert sorted(last["finish"]["seconds"]) == ["finish", "rank"]
        assert all(v > 0 for v in last["finish"]["seconds"].values())
        assert sum(last["finish"]["seconds"].values()) <= last["seconds"]["estimate"]
        assert sorted(last["seconds"]) == ["destripe", "estimate", "read", "write"]
        assert last["planes"] == {"0": 4, "1": 4} and last["quantiles"] == {"flat": 0.5, "dark": 0.05}


def test_the_native_paths_run_destripe_channel(channel):
    root, _, native, *_ = channel
    d = root / "derivatives"
    d.mkdir(exist_ok=True)
    mini_tiff.imwrite(str(d / "DarkMaster_cropped.tif"), np.full((40, 56), 90, np.uint16))
    done = zd.destripe_channel(zarr_dataset_path=root / "data", derivatives_path=d, channel_name=CHANNEL,
                               results_folder=root / "results", xyz_resolution=[1.8, 1.8, 2.0],
                               estimated_channel_flats=native, laser_tiles=SIDES, parameters=PARAMS,
                               prediction_chunksize=(8, 32, 48), output_chunks=(1, 1, 8, 16, 16), compressor="zlib",
                               device=0)  # fmt: skip
    assert done == {name + ".zarr": 16 for name in NAMES}
    out = MiniZarrArray.open(str(root / "results" / "destriped_data" / CHANNEL / (NAMES[0] + ".zarr") / "0"))
    assert out.shape == (1, 1, 16, 32, 48) and out[0, 0].any()


def test_an_odd_plane_is_cropped_on_the_device(tmp_path):
    sides = {"0": [NAMES[0]]}
    vols = _channel(tmp_path, sides, Z=8, H=31, W=47)
    (path,) = fe.estimate_channel_flats(tmp_path / "data", CHANNEL, sides, PARAMS, tmp_path / "flats", plane_step=2, smoothing=1.0,
                                        finish="native")  # fmt: skip
    got = mini_tiff.imread(path)
    assert got.shape == (31, 47) and got.dtype == np.float32
    stack = _host_stack(vols, sides["0"], fe.sampled_planes(8, 8, 1, 2))
    assert stack.shape == (4, 31, 47)
    assert got.tobytes() == fe.estimate_fields(stack, smoothing=1.0, finish="native")["flatfield"].tobytes()


def test_slide_flat_estimation_and_shading_correction_take_the_option(tmp_path, monkeypatch):
    cols, rows, slides = ["431040", "457080"], ["368180", "394100"], ["000000.tif"]
    struct = {CHANNEL: {}}
    for k, (col, row) in enumerate((c, w) for c in cols for w in rows):
        folder = tmp_path / CHANNEL / col / "{}_{}".format(col, row)
        folder.mkdir(parents=True)
        struct[CHANNEL].setdefault(col, {})["{}_{}".format(col, row)] = list(slides)
        plane = np.clip(synth.synthetic_plane(k, 32, 48) * 5.0 * _vignette(32, 48), 0, 65535).astype(np.uint16)
        mini_tiff.imwrite(str(folder / slides[0]), plane)
    monkeypatch.chdir(tmp_path)  # the reference builds its tile paths relative to the channel name
    options = {"smoothing": 1.5, "dark_quantile": 0.25, "finish": "native"}
    r = fe.slide_flat_estimation(struct, CHANNEL, [0], options, synth.NO_CELLS_CONFIG, synth.CELLS_CONFIG)[0]
    want = fe.estimate_fields(np.stack(r["data"]), **options)
    assert r["flatfield"].tobytes() == want["flatfield"].tobytes()
    assert r["darkfield"].tobytes() == want["darkfield"].tobytes()
    today = fe.estimate_fields(np.stack(r["data"]), **dict(options, finish="numpy"))
    assert _adjacent(r["flatfield"], today["flatfield"]) and _adjacent(r["darkfield"], today["darkfield"])
    again = fe.shading_correction(r["data"], options)
    assert again["flatfield"].tobytes() == r["flatfield"].tobytes()
    assert again["darkfield"].tobytes() == r["darkfield"].tobytes()
    numpy_again = fe.shading_correction(r["data"], dict(options, finish="numpy"))
    assert numpy_again["flatfield"].tobytes() == today["flatfield"].tobytes()
    assert numpy_again["darkfield"].tobytes() == today["darkfield"].tobytes()
