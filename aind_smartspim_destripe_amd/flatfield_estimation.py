"""Retrospective flat fields from sampled tile planes (the reference's ``flatfield_estimation.py``).

The reference destripes sample tiles, fits a flat / dark / baseline to them with BaSiC (BaSiCPy) and merges the fits with
``unify_fields``.  BaSiC is NOT restated here and nothing below imitates it.  The estimator of this module is stated by
formulas (:func:`estimate_fields`): a per-pixel quantile of the destriped sample planes -- one order statistic per pixel
across the stack, taken where the planes lie, in device memory (``csrc/dsx_stackrank.h``, integer-exact) -- followed by a
Gaussian smoothing and a normalisation of that one plane: in NumPy on the host (``finish="numpy"``, the default), or
where the rank planes lie (``finish="native"``: ``csrc/dsx_smooth.h``, a float64 contract that the device kernels and a
host build meet bit for bit).  ``unify_fields`` is plain NumPy in the reference and is mirrored exactly.  Not verified
against BaSiCPy: it is not installed where this was built.

Left out: BaSiC itself, fitting weights (``mask``), a per-image baseline (zeros are returned; ``flatfield_correction``
treats ``None`` and zeros alike), more than 512 planes per stack, dtypes other than uint16, several ranks, a sigma
above 64 on the native finish.
"""

import os
import time
from pathlib import Path
from typing import List, Optional

import numpy as np

from . import engine as _engine
from . import mini_tiff
from .mini_zarr import MiniZarrArray
from .readers import imread

MAX_PLANES = _engine.STACK_RANK_MAX_PLANES
ESTIMATOR_OPTIONS = ("flat_quantile", "dark_quantile", "valid_range", "smoothing", "floor", "device", "finish")
FINISH_ROUTES = ("numpy", "native")
# what the last estimate_channel_flats of this process ran: planes per side, valid range, quantiles, seconds per stage
# "finish": the route of the finish and the seconds of the rank and the finish steps, summed over the sides
LAST_ESTIMATE = {}
# what the last estimate_fields of this process ran: {"finish": route, "seconds": {"rank", "finish"}}
LAST_FIELDS = {}


class DeviceStack:
    """``n`` dense uint16 planes ``stored_shape`` in device memory (``d_planes``: a ``DeviceBuffer`` of ``engine`` or a
    device address), of which the top-left ``shape`` is the image: a plane of odd size is stored grown to even, as the
    filter returns it."""

    def __init__(self, engine, d_planes, n, stored_shape, shape=None):
        self.engine, self.d_planes, self.n = engine, d_planes, int(n)
        self.stored_shape = (int(stored_shape[0]), int(stored_shape[1]))
        self.shape = self.stored_shape if shape is None else (int(shape[0]), int(shape[1]))
        if not (0 < self.shape[0] <= self.stored_shape[0] and 0 < self.shape[1] <= self.stored_shape[1]):
            raise ValueError("DeviceStack: shape {} does not lie inside the stored planes {}".format(self.shape, self.stored_shape))


def quantile_milli(q, name="quantile"):
    """A quantile given as a float as the per-mille integer the kernel takes: it must equal ``k / 1000`` within 1e-9
    for an integer ``0 <= k <= 1000``, ``ValueError`` otherwise."""
    if isinstance(q, (bool, np.bool_)) or not isinstance(q, (int, float, np.integer, np.floating)):
        raise ValueError("{} must be a number in [0, 1], not {!r}".format(name, q))
    q = float(q)
    k = int(round(q * 1000.0)) if np.isfinite(q) else -1
    if not (0 <= k <= 1000) or abs(q - k / 1000.0) > 1e-9:
        raise ValueError("{} must be k / 1000 for an integer 0 <= k <= 1000, not {!r}".format(name, q))
    return k


def _estimator_options(flat_quantile=0.5, dark_quantile=None, valid_range=(0, 65535), smoothing=32.0, floor=0.1, device=0,
                       finish="numpy"):
    """The options of :func:`estimate_fields`, checked (``ValueError``), before any library call."""
    qf = quantile_milli(flat_quantile, "flat_quantile")
    qd = None if dark_quantile is None else quantile_milli(dark_quantile, "dark_quantile")
    _, _, _, lo, hi = _engine.stack_rank_args(1, 1, [qf], valid_range)

    def real(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("{} must be a number, not {!r}".format(name, v))
        return float(v)

    smoothing, floor = real("smoothing", smoothing), real("floor", floor)
    if not (0.0 <= smoothing < np.inf):  # (nan fails both comparisons)
        raise ValueError("smoothing must be 0 or a positive finite sigma in pixels, not {!r}".format(smoothing))
    if not (0.0 < floor < np.inf):
        raise ValueError("floor must be positive and finite, not {!r}".format(floor))
    if isinstance(device, (bool, np.bool_)) or not isinstance(device, (int, np.integer)) or device < 0:
        raise ValueError("device must be a GPU index, not {!r}".format(device))
    if not isinstance(finish, str) or finish not in FINISH_ROUTES:
        raise ValueError("finish must be one of {}, not {!r}".format(list(FINISH_ROUTES), finish))
    if finish == "native" and smoothing > _engine.GAUSS_MAX_SIGMA:
        raise ValueError("finish='native' takes a smoothing of at most {} pixels, not {!r}: use finish='numpy'".format(
            _engine.GAUSS_MAX_SIGMA, smoothing))  # fmt: skip
    return {"flat_quantile": qf, "dark_quantile": qd, "valid_range": (lo, hi), "smoothing": smoothing, "floor": floor,
            "device": int(device), "finish": finish}  # fmt: skip


def _check_option_names(options):
    unknown = sorted(set(options) - set(ESTIMATOR_OPTIONS))
    if unknown:
        raise TypeError("unknown estimator option(s) {}: BaSiC's parameters are not taken (BaSiC is not restated here); "
                        "the options are {}".format(unknown, list(ESTIMATOR_OPTIONS)))  # fmt: skip


def gaussian_smooth(plane, sigma):
    """``scipy.ndimage.gaussian_filter(plane, sigma)`` at its defaults, restated in NumPy for a 2-D float64 plane:
    separable, radius ``int(4 sigma + 0.5)``, normalised taps, half-sample reflection at the borders
    (``np.pad(mode="symmetric")``, which folds as often as a short axis needs).  ``sigma == 0`` is the identity."""
    a = np.asarray(plane, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("gaussian_smooth takes one 2-D plane")
    sigma = float(sigma)
    if sigma == 0.0:
        return a.copy()
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    taps = np.exp(-0.5 / (sigma * sigma) * x * x)
    taps /= taps.sum()
    for axis in (0, 1):
        n = a.shape[axis]
        pad = [(0, 0), (0, 0)]
        pad[axis] = (radius, radius)
        padded = np.pad(a, pad, mode="symmetric")
        out = np.zeros_like(a)
        for k in range(2 * radius + 1):
            out += taps[k] * (padded[k : k + n] if axis == 0 else padded[:, k : k + n])
        a = out
    return a


def _rank_planes(stack, q_milli, valid_range):
    """``(R uint16 [n_q, H, W], valid uint16 [H, W])``: the device kernel for a :class:`DeviceStack` (nothing but these
    planes is downloaded), the host build for a host array."""
    if isinstance(stack, DeviceStack):
        eng = stack.engine
        Hs, Ws = stack.stored_shape
        d_out, d_valid = eng.stack_rank(stack.d_planes, stack.n, Hs * Ws, q_milli, valid_range)
        try:
            eng.sync()
            R = d_out.download((len(q_milli), Hs, Ws), np.uint16)
            valid = d_valid.download((Hs, Ws), np.uint16)
        finally:
            d_out.free()
            d_valid.free()
        H, W = stack.shape
        return np.ascontiguousarray(R[:, :H, :W]), np.ascontiguousarray(valid[:H, :W]), stack.n
    a = np.asarray(stack)
    if a.ndim != 3 or a.dtype != np.uint16:
        raise ValueError("estimate_fields takes a uint16 stack [n, H, W] or a DeviceStack, got {} {}".format(a.dtype, a.shape))
    R, valid = _engine.stack_rank_ref(a, q_milli, valid_range)
    return R, valid, a.shape[0]


def _native_fields(stack, q_milli, opt):
    """Rank and native finish: ``(flat, dark, valid, n, seconds of the rank step, seconds of the finish)``.  A
    :class:`DeviceStack` is ranked and finished on the device and only ``flat``, ``dark`` and ``valid`` are downloaded; a
    host array goes through the two host builds."""
    _, taps = _engine.gauss_taps(opt["smoothing"])
    if isinstance(stack, DeviceStack):
        eng = stack.engine
        Hs, Ws = stack.stored_shape
        H, W = stack.shape
        t0 = time.perf_counter()
        d_out, d_valid = eng.stack_rank(stack.d_planes, stack.n, Hs * Ws, q_milli, opt["valid_range"])
        d_flat = d_dark = None
        try:
            eng.sync()
            t1 = time.perf_counter()
            d_flat, d_dark = eng.flat_finish(d_out, d_valid, (Hs, Ws), (H, W), len(q_milli), taps, opt["floor"])
            t2 = time.perf_counter()
            flat = d_flat.download((H, W), np.float32)
            dark = None if d_dark is None else d_dark.download((H, W), np.float32)
            valid = np.ascontiguousarray(d_valid.download((Hs, Ws), np.uint16)[:H, :W])
        finally:
            for d in (d_out, d_valid, d_flat, d_dark):
                if d is not None:
                    d.free()
        return flat, dark, valid, stack.n, t1 - t0, t2 - t1
    t0 = time.perf_counter()
    R, valid, n = _rank_planes(stack, q_milli, opt["valid_range"])
    t1 = time.perf_counter()
    flat, dark = _engine.flat_finish_ref(R, valid, valid.shape, taps, opt["floor"])
    return flat, dark, valid, n, t1 - t0, time.perf_counter() - t1


def estimate_fields(stack_or_device_stack, *, flat_quantile=0.5, dark_quantile=None, valid_range=(0, 65535),
                    smoothing=32.0, floor=0.1, device=0, finish="numpy"):  # fmt: skip
    """Flat (and dark) field of a stack of destriped uint16 planes ``[n, H, W]``, ``n <= 512``.

    1. ``R_flat`` (and ``R_dark``): per pixel the ``flat_quantile`` (``dark_quantile``) of the values inside
       ``valid_range = (lo, hi)``, ``m`` of them, by the integer rank rule ``k = (q_milli * (m - 1)) // 1000``; ``valid``
       = ``m``.  A quantile must be ``k / 1000`` within 1e-9.  One ``stack_rank`` call: on the device for a
       :class:`DeviceStack` (only these ``[H, W]`` planes are downloaded), the host build of the same contract for a
       host array (no GPU involved; ``device`` is then not used).
    2. Pixels with ``valid == 0`` take ``np.median`` of ``R`` over the other pixels (float64); ``ValueError`` if no pixel
       is valid.
    3. ``S = G(float64(R_flat), smoothing)``, ``G`` = :func:`gaussian_smooth`.
    4. ``flatfield = float32(max(S / mean(S), floor))``; ``darkfield = float32(G(R_dark))`` when asked for, else ``None``.
    5. ``baseline``: float32 zeros ``[n]`` (BaSiC's per-image baseline is left out).

    ``finish``: who runs steps 2 to 4.  ``"numpy"`` (the default): the lines above, in NumPy on the host.  ``"native"``:
    the native finish of ``include/dsx.h`` -- the same steps with every float64 operation fixed (explicit fused
    multiply-adds over the taps' centre and right half, the mean summed in 4096 strided lanes), ``smoothing <= 64``; on
    the device, behind the rank kernel, for a :class:`DeviceStack` (only ``flat``, ``dark`` and ``valid`` are
    downloaded), and by the host build of the same contract for a host array: the two agree bit for bit, and differ
    from ``"numpy"`` by at most one float32 spacing.  :data:`LAST_FIELDS` records the route and the seconds of the rank
    and the finish steps.

    Returns ``{"flatfield", "darkfield", "baseline", "valid"}``."""
    opt = _estimator_options(flat_quantile, dark_quantile, valid_range, smoothing, floor, device, finish)
    q = [opt["flat_quantile"]] + ([] if opt["dark_quantile"] is None else [opt["dark_quantile"]])
    if opt["finish"] == "native":
        try:
            flat, dark, valid, n, t_rank, t_finish = _native_fields(stack_or_device_stack, q, opt)
        except _engine.NoSeenPixel:
            raise ValueError("estimate_fields: no pixel has a value inside valid_range {}".format(opt["valid_range"])) from None
        LAST_FIELDS.clear()
        LAST_FIELDS.update({"finish": "native", "seconds": {"rank": t_rank, "finish": t_finish}})
        return {"flatfield": flat, "darkfield": dark, "baseline": np.zeros(n, np.float32), "valid": valid}
    t0 = time.perf_counter()
    R, valid, n = _rank_planes(stack_or_device_stack, q, opt["valid_range"])
    t1 = time.perf_counter()
    seen = valid > 0
    if not seen.any():
        raise ValueError("estimate_fields: no pixel has a value inside valid_range {}".format(opt["valid_range"]))
    planes = []
    for r in R:
        r = r.astype(np.float64)
        if not seen.all():
            r[~seen] = np.median(r[seen])
        planes.append(gaussian_smooth(r, opt["smoothing"]))
    S = planes[0]
    flat = np.maximum(S / S.mean(), opt["floor"]).astype(np.float32)
    dark = planes[1].astype(np.float32) if len(planes) > 1 else None
    LAST_FIELDS.clear()
    LAST_FIELDS.update({"finish": "numpy", "seconds": {"rank": t1 - t0, "finish": time.perf_counter() - t1}})
    return {"flatfield": flat, "darkfield": dark, "baseline": np.zeros(n, np.float32), "valid": valid}


def shading_correction(slides: List[np.array], shading_parameters: dict, mask: Optional[np.array] = None):
    """``flatfield_estimation.py:15-52`` with this module's estimator in BaSiC's place: ``slides`` (uint16 planes of one
    shape, at most 512) are put on the device and ranked there; ``shading_parameters`` are the keyword arguments of
    :func:`estimate_fields` (an unknown key is a ``TypeError``: BaSiC's parameters are not taken); a ``mask`` is a
    ``ValueError`` (fitting weights are left out).  Returns the reference's three keys."""
    if mask is not None:
        raise ValueError("shading_correction: fitting weights (mask) are left out of this estimator")
    params = dict(shading_parameters or {})
    _check_option_names(params)
    opt = _estimator_options(**params)
    a = np.asarray(slides)
    if a.ndim != 3 or a.dtype != np.uint16 or not (1 <= a.shape[0] <= MAX_PLANES):
        raise ValueError("shading_correction takes 1 .. {} uint16 planes of one shape, got {} {}".format(MAX_PLANES, a.dtype, a.shape))
    eng = _engine.DestripeEngine(opt["device"])
    try:
        d = eng.alloc(max(a.nbytes, 16))
        d.upload(a)
        res = estimate_fields(DeviceStack(eng, d, a.shape[0], a.shape[1:]), **params)
    finally:
        eng.close()
    return {"flatfield": res["flatfield"], "darkfield": res["darkfield"], "baseline": res["baseline"]}


def unify_fields(
    flatfields: List[np.array],
    darkfields: List[np.array],
    baselines: List[np.array],
    mode: Optional[str] = "median",
):
    """``flatfield_estimation.py:55-122``, exactly: median / mean over the fields, or ``"mip"`` (max of the flats and
    baselines, min of the darks); float16 results."""
    flatfields = np.array(flatfields)
    darkfields = np.array(darkfields)
    baselines = np.array(baselines)

    if mode == "median":
        flatfield = np.median(flatfields, axis=0)
        darkfield = np.median(darkfields, axis=0)
        baseline = np.median(baselines, axis=0)
    elif mode == "mean":
        flatfield = np.mean(flatfields, axis=0)
        darkfield = np.mean(darkfields, axis=0)
        baseline = np.mean(baselines, axis=0)
    elif mode == "mip":
        flatfield = np.max(flatfields, axis=0)
        darkfield = np.min(darkfields, axis=0)
        baseline = np.max(baselines, axis=0)
    else:
        raise NotImplementedError("Accepted values are: ['mean', 'median', 'mip']")

    return flatfield.astype(np.float16), darkfield.astype(np.float16), baseline.astype(np.float16)


class _At:
    """A device address where the engine calls take a buffer."""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


def _configs(parameters):
    try:
        return parameters["cells_config"], parameters["no_cells_config"]
    except (KeyError, TypeError):
        raise ValueError("parameters must hold 'cells_config' and 'no_cells_config'") from None


def _destripe_into(eng, planes, d_in, d_stack, first, stored_elems):
    """Uploads ``planes[k, H, W]`` (uint16) and destripes them, unshaded, as uint16 into planes ``first ..`` of the stack."""
    d_in.upload(planes)
    at = _At(d_stack.ptr + 2 * first * stored_elems, d_stack.nbytes - 2 * first * stored_elems)
    eng.run_device(d_in, np.uint16, planes.shape[0], at, np.uint16)


def slide_flat_estimation(
    dict_struct: dict,
    channel_name: str,
    slide_idxs: List[int],
    shading_parameters: dict,
    no_cells_config,
    cells_config,
) -> dict:
    """``flatfield_estimation.py:125-196``: per slide of ``slide_idxs`` every tile ``<channel>/<col>/<col>_<row>/<slide>``
    of the folder structure is read (``readers.imread``), the tiles are destriped unshaded as uint16 in cohorts, straight
    into one device stack, and :func:`estimate_fields` runs on that stack.  Returns ``{slide_idx: {"flatfield",
    "darkfield", "baseline", "data"}}``, ``"data"`` the downloaded destriped tiles in the reference's order (planes of odd
    size come back grown to even, as ``log_space_fft_filtering`` returns them; the fields have the tile's own shape).
    ``shading_parameters``: as in :func:`shading_correction`."""
    params = dict(shading_parameters or {})
    _check_option_names(params)
    opt = _estimator_options(**params)
    dict_struct = dict_struct[channel_name]
    cols = list(dict_struct.keys())
    rows = [row.split("_")[-1] for row in list(dict_struct[cols[0]].keys())]
    row_name = f"{cols[0]}_{rows[0]}"
    n_tiles = len(cols) * len(rows)
    if n_tiles > MAX_PLANES:
        raise ValueError("slide_flat_estimation: {} tiles per slide, the estimator takes {}".format(n_tiles, MAX_PLANES))

    per_slide = {}
    eng = _engine.DestripeEngine(opt["device"])
    try:
        for slide_idx in slide_idxs:
            slide_name = dict_struct[cols[0]][row_name][slide_idx]
            tiles = []
            for col in cols:
                for row in rows:
                    tiles.append(np.asarray(imread(f"{channel_name}/{col}/{col}_{row}/{slide_name}")))
            tiles = np.stack(tiles)
            if tiles.ndim != 3 or tiles.dtype != np.uint16:
                raise ValueError("slide_flat_estimation takes uint16 tiles of one shape, got {} {}".format(tiles.dtype, tiles.shape))
            H, W = tiles.shape[1:]
            eng.plan(H, W, cells_config, no_cells_config, max_batch=min(32, n_tiles))
            Hs, Ws = eng.out_shape
            d_in, d_stack = eng.alloc(tiles.nbytes), eng.alloc(2 * n_tiles * Hs * Ws)
            try:
                _destripe_into(eng, tiles, d_in, d_stack, 0, Hs * Ws)
                res = estimate_fields(DeviceStack(eng, d_stack, n_tiles, (Hs, Ws), (H, W)), **params)
                data = d_stack.download((n_tiles, Hs, Ws), np.uint16)
            finally:
                d_in.free()
                d_stack.free()
            per_slide[slide_idx] = {"flatfield": res["flatfield"], "darkfield": res["darkfield"],
                                    "baseline": res["baseline"], "data": list(data)}  # fmt: skip
    finally:
        eng.close()
    return per_slide


def _whole(name, v, least=1):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError("{} must be an integer >= {}, not {!r}".format(name, least, v))
    return int(v)


def sampled_planes(z_extent, z_chunk, blocks_per_tile=1, plane_step=8):
    """The z indices :func:`estimate_channel_flats` samples from a tile of ``z_extent`` planes stored in z chunks of
    ``z_chunk``: ``blocks_per_tile`` blocks of one z chunk each, spread evenly over the chunks (block ``i`` is chunk
    ``floor((i + 1/2) * n_chunks / blocks)``, so a single block is the centre one), every ``plane_step``-th plane of a
    block."""
    n_chunks = -(-int(z_extent) // int(z_chunk))
    picked = sorted({min(n_chunks - 1, ((2 * i + 1) * n_chunks) // (2 * blocks_per_tile)) for i in range(blocks_per_tile)})
    out = []
    for c in picked:
        out.extend(range(c * z_chunk, min((c + 1) * z_chunk, z_extent), plane_step))
    return out


def estimate_channel_flats(zarr_dataset_path, channel_name, laser_tiles, parameters, output_folder, *, multiscale="0",
                           blocks_per_tile=1, plane_step=8, microscope_high_int=2700, rotate=False, device=0,
                           **estimator_options):  # fmt: skip
    """The retrospective flats ``destripe_channel`` needs, one per laser side, from the channel's own tiles.

    For every laser side of ``laser_tiles`` (``{side: [tile stems]}``, as ``destripe_channel`` takes it): from every
    ``<channel>/<tile>.zarr/<multiscale>`` of that side, :func:`sampled_planes` are read, destriped on the device with the
    configs of ``parameters`` (``cells_config`` / ``no_cells_config``; unshaded, uint16) into the side's stack, and
    :func:`estimate_fields` (``estimator_options``: its keyword arguments) runs on that stack.  Planes of odd size grow as
    ``log_space_fft_filtering`` grows them; the rank planes are cropped back to ``[H, W]``.  The flat goes to
    ``<output_folder>/estimated_flat_laser_<channel>_<side>.tif`` (float32).  Returns the paths in side order, ready to
    be passed as ``estimated_channel_flats``; :data:`LAST_ESTIMATE` records what ran.

    Before anything is read: an unknown option is a ``TypeError``, a bad one a ``ValueError``; a tile in neither side
    raises the ``ValueError`` of ``destripe_channel``; a side without tiles, tiles of different plane shapes on a side, a
    dtype other than uint16 and more than 512 sampled planes on a side (raise ``plane_step``) are ``ValueError``.  Single
    process."""
    _check_option_names(estimator_options)
    opt = _estimator_options(device=device, **estimator_options)
    estimator_options = dict(estimator_options, device=device)
    rotate = _engine.rotate_flag(rotate)
    blocks_per_tile, plane_step = _whole("blocks_per_tile", blocks_per_tile), _whole("plane_step", plane_step)
    cells_config, no_cells_config = _configs(parameters)
    channel_dataset = Path(zarr_dataset_path).joinpath(channel_name)
    sides = sorted(laser_tiles, key=int)
    per_side = {side: [] for side in sides}
    for tile_path in sorted(channel_dataset.glob("*.zarr")):
        tile_stem = tile_path.stem.rsplit(".", 1)[0]
        for side in sides:
            if tile_stem in laser_tiles[side]:
                per_side[side].append(tile_path)
                break
        else:
            raise ValueError(f"Tile {tile_path} not found in {laser_tiles}")
    plans = {}
    for side in sides:
        if not per_side[side]:
            raise ValueError("laser side {!r} has no tile under {}".format(side, channel_dataset))
        entries, shape = [], None
        for tile_path in per_side[side]:
            arr = MiniZarrArray.open(str(tile_path / str(multiscale)))
            if arr.ndim != 5 or arr.dtype != np.uint16:
                raise ValueError("{}: the estimator takes uint16 arrays [t, c, z, y, x], got {} {}".format(tile_path, arr.dtype, arr.shape))
            if shape is not None and arr.shape[3:] != shape:
                raise ValueError("laser side {!r}: tiles of different plane shapes ({} and {})".format(side, shape, arr.shape[3:]))
            shape = arr.shape[3:]
            entries.append((arr, sampled_planes(arr.shape[2], arr.chunks[2], blocks_per_tile, plane_step)))
        n = sum(len(z) for _, z in entries)
        if n > MAX_PLANES:
            raise ValueError("laser side {!r}: {} sampled planes, the estimator takes {}: raise plane_step (now {}) or lower "
                             "blocks_per_tile (now {})".format(side, n, MAX_PLANES, plane_step, blocks_per_tile))  # fmt: skip
        plans[side] = (entries, shape, n)

    os.makedirs(output_folder, exist_ok=True)
    seconds = {"read": 0.0, "destripe": 0.0, "estimate": 0.0, "write": 0.0}
    finish_seconds = {"rank": 0.0, "finish": 0.0}
    paths = []
    eng = _engine.DestripeEngine(opt["device"])
    try:
        for side in sides:
            entries, (H, W), n = plans[side]
            eng.plan(H, W, cells_config, no_cells_config, microscope_high_int, max_batch=32, rotate=rotate)
            Hs, Ws = eng.out_shape
            most = max(len(z) for _, z in entries)
            d_in, d_stack = eng.alloc(max(2 * most * H * W, 16)), eng.alloc(2 * n * Hs * Ws)
            try:
                first = 0
                for arr, zs in entries:
                    t0 = time.perf_counter()
                    cz, parts = arr.chunks[2], []
                    for c in sorted({z // cz for z in zs}):  # one source z chunk per block
                        block = arr[0, 0, c * cz : min((c + 1) * cz, arr.shape[2])]
                        parts.append(block[[z - c * cz for z in zs if z // cz == c]])
                    planes = np.ascontiguousarray(np.concatenate(parts))
                    t1 = time.perf_counter()
                    _destripe_into(eng, planes, d_in, d_stack, first, Hs * Ws)
                    eng.sync()
                    first += len(zs)
                    seconds["read"] += t1 - t0
                    seconds["destripe"] += time.perf_counter() - t1
                t0 = time.perf_counter()
                res = estimate_fields(DeviceStack(eng, d_stack, n, (Hs, Ws), (H, W)), **estimator_options)
                seconds["estimate"] += time.perf_counter() - t0
                for step in finish_seconds:
                    finish_seconds[step] += LAST_FIELDS["seconds"][step]
            finally:
                d_in.free()
                d_stack.free()
            t0 = time.perf_counter()
            path = os.path.join(str(output_folder), "estimated_flat_laser_{}_{}.tif".format(channel_name, side))
            mini_tiff.imwrite(path, res["flatfield"])
            seconds["write"] += time.perf_counter() - t0
            paths.append(path)
    finally:
        eng.close()
    LAST_ESTIMATE.clear()
    LAST_ESTIMATE.update({"planes": {side: plans[side][2] for side in sides}, "valid_range": opt["valid_range"],
                          "quantiles": {"flat": opt["flat_quantile"] / 1000.0,
                                        "dark": None if opt["dark_quantile"] is None else opt["dark_quantile"] / 1000.0},
                          "seconds": seconds, "paths": list(paths),
                          "finish": {"route": opt["finish"], "seconds": finish_seconds}})  # fmt: skip
    return paths
