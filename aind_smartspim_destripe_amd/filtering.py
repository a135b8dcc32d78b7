"""Drop-in mirror of ``aind_smartspim_destripe.filtering`` whose hot path runs on an MI355X.

Same names, argument meaning and error behaviour as the reference
(``/root/reference/code/aind_smartspim_destripe/filtering.py``):

* :func:`filter_stripes` (reference ``:417-491``) and :func:`log_space_fft_filtering`
  (``:139-224``) ALWAYS run through the HIP engine (``libdsx_hip.so``); there is no CPU
  fallback -- without the library or a GPU they raise :class:`~.engine.DsxError`.
* :func:`filter_streaks` is the name BASELINE.json's north star keeps (upstream pystripe's): a scalar ``sigma``
  forwards to :func:`log_space_fft_filtering`; ``sigma = (fg, bg)`` runs the dual-band wavelet-FFT filter built from
  the reference's ``foreground_fraction`` / ``gaussian_filter`` helpers (:func:`destripe_streaks_planes` batched).
* :func:`destripe_planes` is the batched form the Zarr chunk map uses instead of the per-plane
  z-loop of ``execute_worker`` (``zarr_destriper.py:319-327``).
* :func:`get_foreground_background_mean` (``:54-88``) and :func:`flatfield_correction` (``:338-414``) called
  on their own also run on the device (``dsx_foreground_background``, ``dsx_flatfield_correction``).
* The remaining helpers (``sigmoid``, ``notch``, ``gaussian_filter``, ``normalize_image``,
  ``get_hemisphere_flatfield``) are parameter / lookup helpers, plain NumPy here as they are there; the
  filter never calls them (the engine builds its own gain tables).
"""

import collections
import math
import warnings
from typing import List, Optional, Tuple

import numpy as np

from . import engine as _engine
from . import wavelets as _wavelets



# ---------------------------------------------------------------------------------------------
# host-side helpers with the reference's names
# ---------------------------------------------------------------------------------------------
def sigmoid(data: np.array):
    """``filtering.py:13-22``."""
    return 1 / (1 + np.exp(-data))


def foreground_fraction(img: np.array, center: float, crossover: float) -> float:
    """``filtering.py:25-51``."""
    z = (img - center) / crossover
    return sigmoid(z)


def _foreground_cutoff(threshold_mask):
    """Smallest float16 pixel value v with ``sigmoid((v - 400) / 20) > threshold_mask`` in the reference's
    float16 arithmetic (``filtering.py:75-78``), found by evaluating every finite float16 value; ``inf`` when
    no pixel value passes.  The decision is monotone in v, so ``float16(pixel) >= cutoff`` is the mask."""
    v = np.arange(0x0000, 0x7C00, dtype=np.uint16).view(np.float16)  # non-negative finite values, ascending
    v = np.concatenate([-v[:0:-1], v])  # negative ones (descending bit pattern = ascending value) first
    with np.errstate(over="ignore"):
        ok = foreground_fraction(v, 400, 20) > threshold_mask
    if not ok.any():
        return float("inf")
    if ok.all():
        return -float("inf")
    first = int(np.argmax(ok))
    if not ok[first:].all():  # not monotone for this threshold (cannot happen for a sigmoid)
        raise ValueError("threshold_mask does not define a cutoff")
    return float(v[first])


def get_foreground_background_mean(img: np.array, threshold_mask: Optional[float] = 0.3, device: int = 0) -> Tuple:
    """``filtering.py:54-88`` on the GPU (``dsx_foreground_background``): (foreground mean, background mean,
    float16 mask image).  ``filter_stripes`` evaluates the same statistic fused into its first kernel.
    """
    img = np.asarray(img)
    if img.size == 0:
        return 0.0, 0.0, np.zeros(img.shape, np.float16)
    cutoff = _foreground_cutoff(threshold_mask)
    eng = next((e[0] for k, e in _ENGINES.items() if k[0] == device), None)
    own = eng is None
    if own:
        eng = _engine.DestripeEngine(device)
    try:
        fore, back, mask = eng.foreground_background(_as_plane_dtype(img), cutoff)
    finally:
        if own:
            eng.close()
    return fore, back, mask.astype(np.float16)


def notch(n, sigma):
    """``filtering.py:91-115``: 1-D gaussian notch ``1 - exp(-x^2 / (2 sigma^2))``."""
    if n <= 0:
        raise ValueError("n must be positive")
    n = int(n)
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    x = np.arange(n)
    return 1 - np.exp(-(x**2) / (2 * sigma**2))


def gaussian_filter(shape, sigma):
    """``filtering.py:118-136``."""
    g = notch(n=shape[-1], sigma=sigma)
    return np.broadcast_to(g, shape).copy()


def normalize_image(images: List[np.array]) -> np.ndarray:
    """``filtering.py:227-250``: scale into [1, 2] (float16 fraction)."""
    images = np.array(images)
    min_val, max_val = np.min(images), np.max(images)
    return 1 + np.divide(images - min_val, max_val - min_val).astype(np.float16)


def invert_image(image: np.array) -> np.ndarray:
    """``filtering.py:253-270``."""
    image = np.array(image)
    return image.max() - image


def get_hemisphere_flatfield(input_tile_path, tile_config, flatfields, zarr=True):
    """``filtering.py:273-335``: flat of the laser side a tile belongs to (``KeyError`` if unknown)."""
    if zarr:
        parts = str(input_tile_path).split("_")
    else:
        parts = str(input_tile_path).split("/")[-2].split("_")
    x_folder, y_folder = parts[0], parts[1]
    if tile_config.get(x_folder) is None:
        raise KeyError(f"Please, check the tile config while trying to reach: {x_folder}")
    brain_side = tile_config[x_folder].get(y_folder)
    if brain_side is None:
        raise KeyError(f"Please, check the tile config while trying to reach: {y_folder}")
    return flatfields[brain_side]


def flatfield_correction(image_tiles, flatfield, darkfield, baseline=None, device=0):
    """``filtering.py:338-414`` as a stand-alone call on the GPU (``dsx_flatfield_correction``; uint16 result).

    Shape handling and errors follow the reference line by line (including its quirk that only one plane
    passes the shape checks, ``:370-391``); the arithmetic runs in float32 on the device.  Inside
    :func:`filter_stripes` the same arithmetic is fused into the last synthesis kernel.
    """
    image_tiles = np.array(image_tiles)
    flatfield, darkfield = np.asarray(flatfield), np.asarray(darkfield)
    if image_tiles.ndim != flatfield.ndim:
        flatfield = np.expand_dims(flatfield, axis=0)
    if image_tiles.ndim != darkfield.ndim:
        darkfield = np.expand_dims(darkfield, axis=0)
    darkfield = darkfield[: image_tiles.shape[-2], : image_tiles.shape[-1]]
    if darkfield.shape != image_tiles.shape:
        raise ValueError(
            "Please, check the shape of the darkfield. "
            f"Image: {image_tiles.shape} - Darkfield: {darkfield.shape}"
        )
    if flatfield.shape != image_tiles.shape:
        raise ValueError(
            "Please, check the shape of the flatfield."
            f"Image: {image_tiles.shape} - Flatfield: {flatfield.shape}"
        )
    if baseline is None:
        baseline = np.zeros((image_tiles.shape[0],))
    baseline = np.asarray(baseline, dtype=np.float64).ravel()
    plane_shape = image_tiles.shape[-2:]
    if image_tiles.ndim < 2 or int(np.prod(image_tiles.shape[:-2])) != 1:
        raise ValueError("flatfield_correction takes one plane ([H, W] or [1, H, W])")
    # baseline[baseline_indxs] (:393-398, 409): index 0 of the array gets one value each -- the rows of a 2-D plane
    # (k_shade takes one value per row), the single plane of a [1, H, W] stack (a scalar)
    if baseline.size not in (1, image_tiles.shape[0]):
        raise ValueError(
            "operands could not be broadcast together with shapes {} {}".format(
                image_tiles.shape, (baseline.size,) + (1,) * (image_tiles.ndim - 1)))
    per_row = image_tiles.ndim == 2 and baseline.size == plane_shape[0] and baseline.size > 1
    eng = next((e[0] for k, e in _ENGINES.items() if k[0] == device), None)
    own = eng is None
    if own:
        eng = _engine.DestripeEngine(device)
    try:
        out = eng.flatfield_correction(_as_plane_dtype(image_tiles.reshape(plane_shape)), flatfield.reshape(plane_shape),
                                       darkfield.reshape(plane_shape),
                                       baseline if per_row else (float(baseline[0]) if baseline.size else 0.0))
    finally:
        if own:
            eng.close()
    return out.reshape(image_tiles.shape)


# ---------------------------------------------------------------------------------------------
# GPU hot path
# ---------------------------------------------------------------------------------------------
_ENGINES = collections.OrderedDict()
_MAX_CACHED_PLANS = 8


def _cfg_key(cfg):
    return (cfg.get("wavelet", "db3"), cfg.get("level", 0), float(cfg.get("sigma", 64)),
            float(cfg.get("max_threshold", 4)))  # fmt: skip


def _max_level(shape, filter_len=6):
    """``pywt.dwt_max_level`` over both axes (6 taps: db3)."""

    def one(n):
        if n < filter_len - 1:
            return 0
        return max(0, int(math.floor(math.log2(n // (filter_len - 1)))))

    return min(one(shape[0]), one(shape[1]))


def _warn_levels(shape, *cfgs):
    """pywt.wavedec2 warns (does not fail) when ``level`` exceeds the maximum useful level."""
    for cfg in cfgs:
        mx = _max_level(shape, _wavelets.filter_length(cfg.get("wavelet", "db3")))
        lvl = cfg.get("level", 0)
        if lvl is not None and lvl > mx:
            warnings.warn(
                f"Level value of {lvl} is too high: all coefficients will experience boundary effects.",
                UserWarning,
            )
        if lvl is not None and lvl < 0:
            raise ValueError("Level value of %d is too low . Minimum level is 0." % lvl)


def get_engine(shape, cells_config, no_cells_config, microscope_high_int=2700, flatfield=None,
               darkfield=None, max_batch=32, device=0, rotate=False):  # fmt: skip
    """Planned engine for a plane geometry + config pair (cached per process and device).  ``rotate``: the plan
    filters vertical stripes (``DestripeEngine.plan``); ``shape`` and the shading planes stay the caller's."""
    rotate = _engine.rotate_flag(rotate)
    shade_key = None
    if flatfield is not None:
        # keyed on the memory the planes occupy, not on the Python object: ``flatfields[brain_side]`` makes a new
        # view object per call (prospective flats, filtering.py:478), which would miss the cache every time
        shade_key = (_array_key(flatfield), _array_key(darkfield))
    key = (device, tuple(shape), _cfg_key(cells_config), _cfg_key(no_cells_config),
           float(microscope_high_int), shade_key, int(max_batch), rotate)  # fmt: skip
    eng = _ENGINES.get(key)
    if eng is not None:
        _ENGINES.move_to_end(key)  # least recently used entries go first
        return eng[0]
    while len(_ENGINES) >= _MAX_CACHED_PLANS:
        _, old = _ENGINES.popitem(last=False)
        old[0].close()
    e = _engine.DestripeEngine(device)
    e.plan(shape[0], shape[1], cells_config, no_cells_config, microscope_high_int, max_batch,
           flatfield, darkfield, rotate=rotate)  # fmt: skip
    # the shading arrays stay referenced, so their addresses stay unique while the plan is cached
    _ENGINES[key] = (e, flatfield, darkfield)
    return e


def release_engines():
    """Close every cached engine of this process (their workspaces go back to the device; a later call plans anew and
    its context reads the ``DSX_*`` switches of the environment again)."""
    while _ENGINES:
        _, old = _ENGINES.popitem(last=False)
        old[0].close()


def _array_key(a):
    a = np.asarray(a)
    return (a.__array_interface__["data"][0], a.shape, a.strides, a.dtype.str)


def _as_plane_dtype(image):
    image = np.asarray(image)
    if image.dtype == np.uint16 or image.dtype == np.float32:
        return np.ascontiguousarray(image)
    if np.issubdtype(image.dtype, np.integer) and image.size and image.min() >= 0 and image.max() <= 65535:
        return np.ascontiguousarray(image, dtype=np.uint16)
    return np.ascontiguousarray(image, dtype=np.float32)


def log_space_fft_filtering(
    input_image: np.array,
    wavelet: Optional[str] = "db3",
    level: Optional[int] = 0,
    sigma: Optional[int] = 64,
    max_threshold: Optional[int] = 4,
    *,
    rotate: bool = False,
):
    """``filtering.py:139-224`` on the GPU: log -> DWT (any PyWavelets discrete wavelet but ``dmey``; ``db3``,
    the production setting, has specialised kernels) -> per-level Otsu mask, row-median
    in-paint and packed-index gaussian notch on cH -> inverse DWT -> ``exp(.) + 1.0``.

    Returns float64 ``[H + H % 2, W + W % 2]`` like the reference (computed in float32 on the
    device; within 1e-4 relative of the NumPy/SciPy path).

    A 3-D ``[n, H, W]`` input is the reference's stack mode (``:182-183, 188, 210-211``): every plane is decomposed
    on its own, but each level takes ONE Otsu threshold from the coefficients of all planes (``dsx_set_stack_mode``).
    Planes that are to be filtered independently go through :func:`destripe_planes`.

    ``rotate=True`` filters vertical stripes: ``np.rot90(F(np.rot90(x)), -1)`` per plane, ``F`` this call without the
    option; the turns run on the device (``dsx_set_rotate``).
    """
    rotate = _engine.rotate_flag(rotate)
    image = np.asarray(input_image)
    if image.ndim not in (2, 3):
        raise ValueError("log_space_fft_filtering takes a 2-D plane or a 3-D stack [n, H, W]")
    cfg = {"wavelet": wavelet, "level": level, "sigma": sigma, "max_threshold": max_threshold}
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    _warn_levels(image.shape[-2:], cfg)
    if image.ndim == 3:
        if image.shape[0] == 0:
            raise ValueError("empty stack")
        planes = image if image.dtype in (np.uint16, np.float32) else np.stack([_as_plane_dtype(p) for p in image])
        if planes.dtype not in (np.uint16, np.float32):
            planes = planes.astype(np.float32)
        eng = get_engine(image.shape[-2:], cfg, cfg, microscope_high_int=2700, max_batch=int(image.shape[0]),
                         rotate=rotate)
        eng.set_stack_mode(True)
        try:
            out = eng.run(np.ascontiguousarray(planes), out_dtype=np.float32)
        finally:
            eng.set_stack_mode(False)
        return out.astype(np.float64)
    eng = get_engine(image.shape, cfg, cfg, microscope_high_int=2700, max_batch=1, rotate=rotate)
    out = eng.run(_as_plane_dtype(image)[None], out_dtype=np.float32)[0]
    return out.astype(np.float64)


def _streaks_params(sigma, level, wavelet, crossover, threshold):
    """Checks of the dual-band form (every one before any device call); returns (sigma_fg, sigma_bg, level).  One
    member of the pair may be ``None``: that band is not filtered (the blend takes the raw plane in its place)."""
    if isinstance(sigma, (str, bytes)) or not isinstance(sigma, (tuple, list, np.ndarray)) or len(sigma) != 2 \
            or any(v is not None and np.ndim(v) != 0 for v in sigma):  # fmt: skip
        raise ValueError("sigma must be a number or a pair (sigma_fg, sigma_bg)")
    if sigma[0] is None and sigma[1] is None:
        raise ValueError("sigma: at least one of (sigma_fg, sigma_bg) must be a number")
    sigma_fg, sigma_bg = (None if v is None else float(v) for v in sigma)
    if not all(v is None or v > 0 for v in (sigma_fg, sigma_bg)):
        raise ValueError("sigma must be positive")
    if not (float(crossover) > 0):
        raise ValueError("crossover must be positive")
    if threshold is None or not np.isfinite(float(threshold)):
        raise ValueError("threshold must be -1 (Otsu) or a finite value")
    if level is not None and level < 0:
        raise ValueError("Level value of %d is too low . Minimum level is 0." % level)
    _wavelets.filter_bank(_engine._wavelet_key({"wavelet": wavelet}))  # ValueError for names the engine refuses
    return sigma_fg, sigma_bg, 0 if level is None else int(level)


def _streaks_engine(shape, sigma_fg, sigma_bg, level, wavelet, crossover, threshold, max_batch, device,
                    route="generic", smoothing=0.0, flat=None, dark=None, rotate=False):  # fmt: skip
    """Planned streaks engine (cached per process and device); ``route`` is resolved: ``generic`` or ``march``.
    ``sigma_fg`` / ``sigma_bg``: one may be ``None`` (a one-sided plan).  ``rotate``: as in :func:`get_engine`."""
    rotate = _engine.rotate_flag(rotate)
    fixed = None if float(threshold) == -1 else float(threshold)
    shade_key = None if flat is None else (_array_key(flat), _array_key(dark))
    key = (device, "streaks", tuple(shape), sigma_fg, sigma_bg, level, _engine._wavelet_key({"wavelet": wavelet}),
           float(crossover), fixed, int(max_batch), route, float(smoothing), shade_key, rotate)  # fmt: skip
    eng = _ENGINES.get(key)
    if eng is not None:
        _ENGINES.move_to_end(key)
        return eng[0]
    while len(_ENGINES) >= _MAX_CACHED_PLANS:
        _, old = _ENGINES.popitem(last=False)
        old[0].close()
    e = _engine.DestripeEngine(device)
    bands = "fg" if sigma_bg is None else "bg" if sigma_fg is None else "both"
    e.plan_streaks(shape[0], shape[1], sigma_bg if sigma_fg is None else sigma_fg,
                   sigma_fg if sigma_bg is None else sigma_bg, wavelet=wavelet, level=level, crossover=crossover,
                   threshold=fixed, max_batch=max_batch, route=route, bands=bands, smoothing=smoothing, flatfield=flat,
                   darkfield=dark, rotate=rotate)  # fmt: skip
    # (the shading arrays stay referenced, so their addresses stay unique while the plan is cached)
    _ENGINES[key] = (e, flat, dark)
    return e


STREAKS_DEFAULTS = {"sigma": None, "level": 0, "wavelet": "db3", "crossover": 10, "threshold": -1, "route": "auto"}
# optional keys of the ``streaks=`` dict: passed through (checked) only when present
STREAKS_OPTIONAL = ("smoothing", "shading", "rotate")


def streaks_options(streaks):
    """The ``streaks=`` dict of the pipelines (``destripe_zarr_store``, ``destripe_zarr``, ``batch_filter``), checked
    and completed with the defaults of :func:`filter_streaks` (``route``: ``"auto"``): ``TypeError`` for an unknown key
    or a missing ``sigma`` pair, ``ValueError`` for a bad value.  The optional keys ``"smoothing"`` (0 or
    ``0 < s <= 2``) and ``"shading"`` (a bool: apply the pipeline's ``shadow_correction`` to the filter's result) are
    in the result only when they were given; so is ``"rotate"`` (a bool, ``TypeError`` for anything else: the filter
    runs on ``np.rot90`` of every plane and the result is turned back -- vertical stripes).  No device call."""
    if not isinstance(streaks, dict):
        raise TypeError("streaks must be a dict {'sigma': (fg, bg), ...}")
    unknown = sorted(set(streaks) - set(STREAKS_DEFAULTS) - set(STREAKS_OPTIONAL))
    if unknown:
        raise TypeError("streaks got unexpected keys: {}".format(unknown))
    opt = dict(STREAKS_DEFAULTS, **streaks)
    if opt["sigma"] is None:
        raise TypeError("streaks needs 'sigma': (sigma_fg, sigma_bg)")
    if opt["route"] not in ("generic", "march", "auto"):
        raise ValueError("route must be 'generic', 'march' or 'auto', not {!r}".format(opt["route"]))
    sigma_fg, sigma_bg, opt["level"] = _streaks_params(opt["sigma"], opt["level"], opt["wavelet"], opt["crossover"],
                                                       opt["threshold"])  # fmt: skip
    opt["sigma"] = (sigma_fg, sigma_bg)
    if "smoothing" in opt:
        opt["smoothing"] = _engine.streaks_smoothing(opt["smoothing"])
    if "shading" in opt:
        if not isinstance(opt["shading"], (bool, np.bool_)):
            raise ValueError("shading must be True or False")
        opt["shading"] = bool(opt["shading"])
    if "rotate" in opt:
        opt["rotate"] = _engine.rotate_flag(opt["rotate"])
    return opt


def streaks_call_options(streaks, flat=None, dark=None):
    """The keyword arguments of :func:`destripe_streaks_planes` / :func:`filter_streaks` for a checked ``streaks``
    dict: the ``"shading"`` flag becomes the resolved ``flat`` / ``dark`` planes (dropped when it is not set)."""
    kw = {k: v for k, v in streaks.items() if k != "shading"}
    if streaks.get("shading") and flat is not None:
        kw["flat"], kw["dark"] = flat, dark
    return kw


def streaks_shading(streaks, shadow_correction):
    """``shadow_correction`` as a streaks pipeline takes it: ``None`` when there is none, ``ValueError`` when there is
    one and the checked ``streaks`` dict does not ask for it with ``"shading": True``."""
    if shadow_correction is not None and not streaks.get("shading"):
        raise ValueError("streaks: the dual-band filter has no dark / flat step without 'shading': True; "
                         "shadow_correction must be None")  # fmt: skip
    return shadow_correction


def _warn_streaks_level(shape, level, wavelet):
    padded = [s + (s & 1) for s in shape]
    mx = _max_level((min(padded), min(padded)), _wavelets.filter_length(_engine._wavelet_key({"wavelet": wavelet})))
    if level > mx:
        warnings.warn(
            f"Level value of {level} is too high: all coefficients will experience boundary effects.", UserWarning
        )


def filter_streaks(image, sigma=64, level=0, wavelet="db3", crossover=10, threshold=-1, route="generic", smoothing=0,
                   flat=None, dark=None, rotate=False, **params):  # fmt: skip
    """The stripe filter under its upstream (pystripe) name, in two forms.

    * Scalar ``sigma``: ``log_space_fft_filtering(image, sigma=sigma, level=level, wavelet=wavelet, **params)``,
      unchanged (``crossover`` / ``threshold`` are not arguments of that filter).
    * ``sigma = (sigma_fg, sigma_bg)``: the dual-band wavelet-FFT filter on the GPU (``dsx_plan_streaks``).  ``t`` is
      ``threshold``, or skimage's ``threshold_otsu`` of the plane for ``threshold == -1``; the edge-padded plane is
      split into ``min(x, t)`` and ``max(x, t)``, each band goes through log(1 + z), ``wavedec2`` (``level`` 0 / None
      = the maximum depth), a packed-index notch on every cH row (``s = cH.shape[0] * sigma / H'``), ``waverec2`` and
      exp(r) - 1, and the bands are blended with ``foreground_fraction(x, t, crossover)``.  Equal sigmas run one band
      on the unclipped plane.  Returns float64 ``[H, W]`` (computed in float32 on the device).  ``route``:
      ``"generic"`` (the default: per-band analysis / synthesis kernels, any wavelet and plane), ``"march"`` (the bands
      run through the marching db3 kernels and the FFT row filter of the log-space engine -- the same filter, for
      db3, planes of even height and width and levels up to the maximum; ``ValueError`` elsewhere) or ``"auto"``
      (``engine.AUTO_ROUTE`` where march applies: the generic route until a same-session measurement shows march
      ahead; generic elsewhere).  Options of this form: one member of ``sigma`` may be ``None`` -- ``(s, None)``
      filters the foreground band only (``f w + x (1 - w)``), ``(None, s)`` the background band only
      (``x w + b (1 - w)``); ``smoothing`` (0, or ``0 < s <= 2``) blends with
      ``scipy.ndimage.gaussian_filter(w, smoothing)`` instead of the raw sigmoid ``w``; ``flat`` / ``dark`` (together)
      put the result through the reference's ``flatfield_correction`` and make the return value uint16, as
      :func:`filter_stripes` does.

    ``rotate=True`` (either form; upstream's ``rotate`` switch of ``read_filter_save``) filters vertical stripes:
    ``np.rot90(F(np.rot90(image)), -1)`` with ``F`` this call without the option, the turns on the device; ``flat`` /
    ``dark`` stay in the orientation of ``image``.
    """
    rotate = _engine.rotate_flag(rotate)
    if sigma is not None and not isinstance(sigma, (str, bytes)) and np.ndim(sigma) == 0:
        if ("crossover" in params or crossover != 10 or threshold != -1 or route != "generic" or smoothing != 0
                or flat is not None or dark is not None):  # fmt: skip
            raise TypeError("crossover / threshold / route / smoothing / flat / dark belong to the dual-band form: "
                            "pass sigma=(sigma_fg, sigma_bg)")  # fmt: skip
        return log_space_fft_filtering(input_image=image, sigma=sigma, level=level, wavelet=wavelet, rotate=rotate,
                                       **params)
    if params:
        raise TypeError("filter_streaks got unexpected arguments: {}".format(sorted(params)))
    sigma_fg, sigma_bg, level = _streaks_params(sigma, level, wavelet, crossover, threshold)
    image = np.asarray(image)
    if image.ndim != 2 or image.size == 0:
        raise ValueError("filter_streaks takes one non-empty 2-D plane; use destripe_streaks_planes for a stack")
    out = destripe_streaks_planes(image[None], (sigma_fg, sigma_bg), level=level, wavelet=wavelet, crossover=crossover,
                                  threshold=threshold, out_dtype=np.float32 if flat is None else np.uint16, max_batch=1,
                                  route=route, smoothing=smoothing, flat=flat, dark=dark, rotate=rotate)  # fmt: skip
    return out[0].astype(np.float64) if flat is None else out[0]


def destripe_streaks_planes(planes, sigma, level=0, wavelet="db3", crossover=10, threshold=-1, out_dtype=np.uint16,
                            max_batch=32, device=0, return_threshold=False, route="generic", smoothing=0, flat=None,
                            dark=None, rotate=False):  # fmt: skip
    """Batched dual-band :func:`filter_streaks` over ``planes[n, H, W]`` (uint16 or float32), every plane on its own
    (with ``threshold=-1`` each takes its own Otsu ``t``).  ``out_dtype`` uint16: clip to [0, 65535] and truncate, as
    the Zarr path stores; float32: the filter's value.  ``return_threshold``: also the per-plane ``t`` (float64).
    ``route``, a ``None`` member of ``sigma``, ``smoothing``, ``flat`` / ``dark``: as in :func:`filter_streaks`; with a
    flat, a float32 output is the clipped value of ``flatfield_correction`` (not truncated).  ``rotate``: as in
    :func:`filter_streaks`; ``t`` does not depend on it."""
    rotate = _engine.rotate_flag(rotate)
    sigma_fg, sigma_bg, level = _streaks_params(sigma, level, wavelet, crossover, threshold)
    smoothing = _engine.streaks_smoothing(smoothing)
    if (flat is None) != (dark is None):
        raise ValueError("flatfield and darkfield must be given together")
    planes = np.asarray(planes)
    if planes.ndim != 3:
        raise ValueError("planes must be [n, H, W]")
    if planes.shape[1] == 0 or planes.shape[2] == 0:
        raise ValueError("planes must not be empty")
    route = _engine.streaks_route(route, planes.shape[1], planes.shape[2], wavelet, level)
    if planes.dtype != np.uint16 and planes.dtype != np.float32:
        planes = np.stack([_as_plane_dtype(p) for p in planes]) if len(planes) else planes.astype(np.float32)
        if planes.dtype not in (np.uint16, np.float32):
            planes = planes.astype(np.float32)
    _warn_streaks_level(planes.shape[1:], level, wavelet)
    n = planes.shape[0]
    max_batch = max(1, min(int(max_batch), max(n, 1)))
    eng = _streaks_engine(planes.shape[1:], sigma_fg, sigma_bg, level, wavelet, crossover, threshold, max_batch, device,
                          route, smoothing, flat, dark, rotate)  # fmt: skip
    out = np.empty(planes.shape, dtype=out_dtype)
    ts = np.zeros(n, dtype=np.float64)
    for start in range(0, n, max_batch):
        stop = min(n, start + max_batch)
        out[start:stop] = eng.run(np.ascontiguousarray(planes[start:stop]), out_dtype=out_dtype)
        if return_threshold:
            ts[start:stop] = [eng.streaks_threshold(k) for k in range(stop - start)]
    return (out, ts) if return_threshold else out


LIGHTSHEET_DEFAULTS = dict(_engine.LIGHTSHEET_DEFAULTS)


def lightsheet_options(lightsheet, streaks=None, shadow_correction=None):
    """The ``lightsheet=`` dict of the pipelines (``read_filter_save``, ``batch_filter``, ``destripe_zarr_store``,
    ``destripe_zarr``), checked and completed with the defaults of :func:`correct_lightsheet`: keys ``percentile``,
    ``artifact_length``, ``background_window_size`` and ``lightsheet_vs_background``, all optional.  ``TypeError`` for
    anything but a dict or for an unknown key, ``ValueError`` for a bad value, for a ``streaks`` dict given together
    with it (one filter per run) and for a ``shadow_correction`` (this mode has no dark / flat step).  No library
    call."""
    if not isinstance(lightsheet, dict):
        raise TypeError("lightsheet must be a dict {'percentile': .25, 'artifact_length': 150, ...}")
    unknown = sorted(set(lightsheet) - set(LIGHTSHEET_DEFAULTS), key=str)
    if unknown:
        raise TypeError("lightsheet got unexpected keys: {}".format(unknown))
    if streaks is not None:
        raise ValueError("lightsheet and streaks cannot be given together: a run applies one filter")
    if shadow_correction is not None:
        raise ValueError("lightsheet: the light-sheet background mode has no dark / flat step; "
                         "shadow_correction must be None")  # fmt: skip
    opt = dict(LIGHTSHEET_DEFAULTS, **lightsheet)
    p, A, B, lam = _engine.lightsheet_params(**opt)
    return dict(percentile=p, artifact_length=A, background_window_size=B, lightsheet_vs_background=lam)


def _lightsheet_engine(shape, p, A, B, lam, max_batch, device, rotate=False):
    """Planned light-sheet engine (cached per process and device).  ``rotate``: as in :func:`get_engine`."""
    key = (device, "lightsheet", tuple(shape), p, A, B, lam, int(max_batch), rotate)
    eng = _ENGINES.get(key)
    if eng is not None:
        _ENGINES.move_to_end(key)
        return eng[0]
    while len(_ENGINES) >= _MAX_CACHED_PLANS:
        _, old = _ENGINES.popitem(last=False)
        old[0].close()
    e = _engine.DestripeEngine(device)
    e.plan_lightsheet(shape[0], shape[1], p, A, B, lam, max_batch=max_batch, rotate=rotate)
    _ENGINES[key] = (e, None, None)
    return e


def correct_lightsheet(image, percentile=0.25, artifact_length=150, background_window_size=200,
                       lightsheet_vs_background=2.0, rotate=False):  # fmt: skip
    """Upstream pystripe's light-sheet background mode (``lightsheet=True``) over one uint16 plane, on the GPU
    (``dsx_plan_lightsheet``): the additive glow a sheet leaves along x is estimated by two windowed percentile filters
    on a fixed log scale and subtracted.

    ``q = floor(255 log2(1 + x) / 16)``; ``ls`` = the ``percentile`` of ``q`` over a 1 x ``artifact_length`` window and
    ``bg`` over a ``background_window_size`` square, both with the arithmetic of scikit-image's ``rank.percentile``
    (windows cut at the border); back on the linear scale (``2 ** (16 v / 255) - 1``) the line estimate is the offset
    unless it exceeds ``lightsheet_vs_background`` times the regional one, which then takes its place; the result is
    ``max(x - offset, 0)``, float32 ``[H, W]``.  ``0 < percentile < 1``, ``artifact_length`` 1 .. 1024,
    ``background_window_size`` 1 .. 255 (``ValueError`` elsewhere, and for a plane that is not uint16).
    ``rotate=True``: ``np.rot90(F(np.rot90(image)), -1)``, the turns on the device.  Not verified against pystripe
    itself (README "Light-sheet background mode")."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("correct_lightsheet takes one 2-D plane; use correct_lightsheet_planes for a stack")
    return correct_lightsheet_planes(image[None], percentile, artifact_length, background_window_size,
                                     lightsheet_vs_background, rotate=rotate, out_dtype=np.float32, max_batch=1)[0]  # fmt: skip


def correct_lightsheet_planes(planes, percentile=0.25, artifact_length=150, background_window_size=200,
                              lightsheet_vs_background=2.0, rotate=False, out_dtype=np.uint16, max_batch=32, device=0):  # fmt: skip
    """Batched :func:`correct_lightsheet` over ``planes[n, H, W]`` (uint16), every plane on its own.  ``out_dtype``
    uint16 (the value truncated; it is in range already) or float32."""
    rotate = _engine.rotate_flag(rotate)
    p, A, B, lam = _engine.lightsheet_params(percentile, artifact_length, background_window_size,
                                             lightsheet_vs_background)  # fmt: skip
    planes = np.asarray(planes)
    if planes.ndim != 3:
        raise ValueError("planes must be [n, H, W]")
    if planes.dtype != np.uint16:
        raise ValueError("lightsheet: planes must be uint16, not {}".format(planes.dtype))
    if planes.shape[1] == 0 or planes.shape[2] == 0:
        raise ValueError("planes must not be empty")
    if np.dtype(out_dtype) not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise ValueError("lightsheet: out_dtype must be uint16 or float32")
    n = planes.shape[0]
    max_batch = max(1, min(int(max_batch), max(n, 1)))
    eng = _lightsheet_engine(planes.shape[1:], p, A, B, lam, max_batch, device, rotate)
    out = np.empty(planes.shape, dtype=out_dtype)
    for start in range(0, n, max_batch):
        stop = min(n, start + max_batch)
        out[start:stop] = eng.run(np.ascontiguousarray(planes[start:stop]), out_dtype=out_dtype)
    return out


def _resolve_shading(shadow_correction, input_tile_path):
    if shadow_correction is None:
        return None, None
    flatfield = shadow_correction.get("flatfield")
    darkfield = shadow_correction.get("darkfield")
    if not shadow_correction.get("retrospective"):
        flatfield = get_hemisphere_flatfield(
            input_tile_path=input_tile_path,
            tile_config=shadow_correction.get("tile_config"),
            flatfields=flatfield,
        )
    return flatfield, darkfield


def filter_stripes(
    image: np.array,
    input_tile_path: str,
    no_cells_config: dict,
    cells_config: dict,
    shadow_correction: Optional[dict] = None,
    microscope_high_int: Optional[int] = 2700,
    *,
    rotate: bool = False,
) -> np.array:
    """``filtering.py:417-491`` on the GPU (one plane).

    The fg/bg statistic, the config choice, the filter and (if given) the dark/flat correction
    all run on the device.  Returns float64 without shading and uint16 with shading, like the
    reference.  ``rotate=True``: vertical stripes, ``np.rot90(F(np.rot90(image)), -1)`` with the shading planes in the
    orientation of ``image`` (:func:`destripe_planes`).
    """
    rotate = _engine.rotate_flag(rotate)
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("filter_stripes takes one 2-D plane; use destripe_planes for a stack")
    flatfield, darkfield = _resolve_shading(shadow_correction, input_tile_path)
    _warn_levels(image.shape, cells_config, no_cells_config)
    plane = _as_plane_dtype(image)[None]
    if _engine._wavelet_key(cells_config) != _engine._wavelet_key(no_cells_config):
        out = _destripe_planes_two_wavelets(plane, no_cells_config, cells_config, microscope_high_int, flatfield, darkfield,
                                            np.uint16 if flatfield is not None else np.float32, 1, False, 0,
                                            rotate)[0]  # fmt: skip
        return out if flatfield is not None else out.astype(np.float64)
    eng = get_engine(image.shape, cells_config, no_cells_config, microscope_high_int, flatfield, darkfield,
                     max_batch=1, rotate=rotate)  # fmt: skip
    if flatfield is not None:
        return eng.run(plane, out_dtype=np.uint16)[0]
    return eng.run(plane, out_dtype=np.float32)[0].astype(np.float64)


def destripe_planes(
    planes: np.ndarray,
    input_tile_path: str,
    no_cells_config: dict,
    cells_config: dict,
    shadow_correction: Optional[dict] = None,
    microscope_high_int: Optional[int] = 2700,
    out_dtype=np.uint16,
    max_batch: int = 32,
    return_config: bool = False,
    device: int = 0,
    rotate: bool = False,
):
    """Batched ``filter_stripes`` over ``planes[n, H, W]`` (uint16 or float32): every plane is
    filtered independently, exactly as the z-loop of ``execute_worker`` does
    (``zarr_destriper.py:319-327``), in cohorts of ``max_batch`` planes per launch chain.

    ``out_dtype`` uint16 = what the Zarr path stores (clip + truncate); float32 = ``exp(y) + 1``.

    ``rotate=True`` filters vertical stripes: per plane ``np.rot90(F(np.rot90(x)), -1)``, ``F`` this call without the
    option -- everything the filter derives from the plane shape is derived from the rotated plane, the flat and the
    dark (cropped to the plane) are applied in the orientation of ``x``, and the config decision does not depend on
    the orientation.  The turns run on the device, inside the launch chain (``dsx_set_rotate``).
    """
    rotate = _engine.rotate_flag(rotate)
    planes = np.asarray(planes)
    if planes.ndim != 3:
        raise ValueError("planes must be [n, H, W]")
    flatfield, darkfield = _resolve_shading(shadow_correction, input_tile_path)
    _warn_levels(planes.shape[1:], cells_config, no_cells_config)
    if planes.dtype != np.uint16 and planes.dtype != np.float32:
        planes = np.stack([_as_plane_dtype(p) for p in planes]) if len(planes) else planes.astype(np.float32)
    if _engine._wavelet_key(cells_config) != _engine._wavelet_key(no_cells_config):
        return _destripe_planes_two_wavelets(planes, no_cells_config, cells_config, microscope_high_int, flatfield,
                                             darkfield, out_dtype, max_batch, return_config, device, rotate)  # fmt: skip
    eng = get_engine(planes.shape[1:], cells_config, no_cells_config, microscope_high_int, flatfield,
                     darkfield, max_batch=max_batch, device=device, rotate=rotate)  # fmt: skip
    return eng.run(planes, out_dtype=out_dtype, return_cfg=return_config)


def _destripe_planes_two_wavelets(planes, no_cells_config, cells_config, microscope_high_int, flatfield, darkfield,
                                  out_dtype, max_batch, return_config, device, rotate=False):
    """The two configs name DIFFERENT wavelets.  One launch chain decomposes a plane before its config is known (the
    fg/bg statistic is fused into the first kernel), so it cannot switch filter banks per plane; the reference decides
    first and decomposes afterwards (``filtering.py:459-467``).  Same order here: the statistic of every plane
    (``dsx_foreground_background``), the reference's decision rule, then one engine per config (both of its slots hold
    that config) over the planes that chose it."""
    n = planes.shape[0]
    cutoff = _foreground_cutoff(0.3)
    which = np.zeros(n, dtype=np.int32)
    probe = get_engine(planes.shape[1:], no_cells_config, no_cells_config, microscope_high_int, flatfield, darkfield,
                       max_batch=max_batch, device=device, rotate=rotate)  # fmt: skip
    for k in range(n):
        fore, back, _ = probe.foreground_background(planes[k], cutoff, want_mask=False)
        which[k] = 1 if (fore > back and fore > microscope_high_int) else 0
    out = None
    for w, cfg in ((0, no_cells_config), (1, cells_config)):
        idx = np.nonzero(which == w)[0]
        if idx.size == 0:
            continue
        eng = get_engine(planes.shape[1:], cfg, cfg, microscope_high_int, flatfield, darkfield,
                         max_batch=max_batch, device=device, rotate=rotate)  # fmt: skip
        res = eng.run(np.ascontiguousarray(planes[idx]), out_dtype=out_dtype)
        if out is None:
            out = np.empty((n,) + res.shape[1:], dtype=res.dtype)
        out[idx] = res
    if out is None:
        out = np.empty((0,) + tuple(s + (s & 1) for s in planes.shape[1:]), dtype=out_dtype)
    return (out, which) if return_config else out
