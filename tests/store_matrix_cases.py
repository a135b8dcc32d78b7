"""The store matrix: the options of the Zarr store pass (``destripe_zarr_store``) driven together over one small volume
that no chunk divides, and what the store must then hold, stated in NumPy.  Shared by ``test_store_matrix_host.py``
(CPU) and ``test_gpu_store_matrix.py``.  Importing this module touches no device; only :func:`exact_level0` calls one.

Geometry.  22 planes of 70 x 100, output chunks (4, 32, 32), input chunks (3, 24, 40), z blocks of 8 planes (4 where the
pyramid does not reduce z, as ``fused_check_blocks`` wants it).  So: z blocks of 8, 8 and 6 planes, the last ending inside
an output z chunk, the second and third starting inside an input chunk; brick rows of 32, 32, 6 and brick columns of 32,
32, 32, 4 (6 / 4 swap axes under ``rotate``); pyramid levels with odd extents, the chunk of the last level clamped to its
shape; a second rank whose z range starts at plane 16 (fused pyramid that reduces z) or 12, not at 0.
``test_store_matrix_host.py`` holds the planner to all of this.

Input.  ``synth.synthetic_stack`` (planes 0, 4, 8 ... carry cells: both stripe configs) plus the row glow of
``lightsheet_cases.glow_plane`` (the light-sheet mode changes pixels).  One input chunk file is deleted after writing, the
store's ``fill_value`` is not 0: those voxels are ``FILL_VALUE`` in every expectation.

Expectations, two tiers for level 0.  Exact: the per-plane API over the whole volume (:func:`exact_level0`).
Independent: the NumPy references of the suite on the planes ``SAMPLED`` (:func:`independent_plane`) -- the first and
last plane and both sides of the block seams.  Everything derived from level 0 (pyramid, histogram, projections, display
window, chunk files) is computed in NumPy from the level 0 the store holds, so no filter tolerance enters.

Tolerances of the independent tier (none is new):
* stripes: at most one count from ``orc.filter_stripes`` truncated to uint16, as ``test_gpu_row_pack.py`` states it;
* light-sheet: ``lightsheet_cases.lightsheet_numpy`` truncated to uint16, exact (the contract is integer-exact);
* streaks: ``streaks_options_oracle.filter_streaks``; the suite's standing ``1e-4 (1 + |ref|)`` on the filter's value
  stays below one count while ``ref < 9000``, so the stored uint16 is held within one count of the truncated reference,
  as ``test_gpu_streaks_options.py::test_uint16_output`` states it (``test_gpu_streaks_store.py`` holds the store to the
  per-plane API exactly and has no tolerance of its own against the NumPy restatement).

Cases.  A pairwise cover (:func:`uncovered_pairs`), not the full product: every value of every option of ``OPTIONS``
occurs with every value of ``rotate`` and with every filter that takes it (``applies``).
"""

import functools
import itertools
import os
from collections import namedtuple

import numpy as np

from aind_smartspim_destripe_amd import synth
from aind_smartspim_destripe_amd.mini_zarr import MiniZarrArray
from oracle import destripe_oracle as orc
from oracle import format_oracle as fo
from tests import lightsheet_cases as lc
from tests import streaks_options_oracle as soo

Z, H, W = 22, 70, 100
OUT_CHUNKS = (1, 1, 4, 32, 32)
IN_CHUNKS = (1, 1, 3, 24, 40)
BLOCK_Z = 8
FILL_VALUE = 300  # of the input store: what a missing chunk reads as
MISSING = (5, 1, 2)  # the input chunk (z, y, x) whose file is deleted: planes 15 .. 17, so two z blocks read it
SAMPLED = (0, 7, 8, 16, 21)
SEED = 5
GLOW = 120  # counts: background + glow stay below the ~380 at which a pixel counts as foreground (select_config)
TILE = "X_0_Y_0"
XYZ = (1.8, 1.9, 2.0)  # x, y, z
LZ4 = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
LIGHTSHEET = dict(percentile=0.25, artifact_length=15, background_window_size=21, lightsheet_vs_background=2.0)
SIGMA = (8.0, 16.0)
STREAKS = {"march": {"sigma": SIGMA, "route": "march"},
           "generic": {"sigma": SIGMA, "route": "generic", "wavelet": "sym4", "smoothing": 1}}  # fmt: skip
CELLS, NO_CELLS, HIGH_INT = synth.CELLS_CONFIG, synth.NO_CELLS_CONFIG, synth.ZARR_PATH_HIGH_INT

Case = namedtuple("Case", "name filter route rotate shading pyramid scale n_levels out codec decode hist proj ranks retile entry")


def _c(name, filt, rotate, shading=False, pyramid=None, scale=None, out="blosc", codec=False, decode=False, hist=True,
       proj="both", ranks=1, retile=True, entry=False, n_levels=None):  # fmt: skip
    filt, _, route = filt.partition(":")
    n_levels = (3 if pyramid else 1) if n_levels is None else n_levels
    return Case(name, filt, route or None, rotate, shading, pyramid, scale, n_levels, out, codec, decode, hist, proj, ranks,
                retile, entry)  # fmt: skip


# out: the output compressor; codec: device_codec; decode: device_decode (the input store is Blosc-zstd for False / True,
# Blosc-LZ4 for "any", plain zlib for "full"); entry: the case also runs through destripe_zarr.
CASES = [
    _c("01-stripes-fused222-runs", "stripes", False, True, "fused", (2, 2, 2), "blosc", "runs", True, True, "both", entry=True),
    _c("02-stripes-rot-fused122", "stripes", True, True, "fused", (1, 2, 2), "blosc", False, False, True, "both", entry=True),
    _c("03-stripes-rot-pipelined212", "stripes", True, False, "pipelined", (2, 1, 2), "blosc", True, "any", False, "output", entry=True),
    _c("04-march-rot-shaded-fused221-lz4", "streaks:march", True, True, "fused", (2, 2, 1), LZ4, True, "any", True, "output", entry=True),
    _c("05-generic-sym4-flat-zlib-in", "streaks:generic", False, False, None, None, "zlib", False, "full", True, "both", entry=True),
    _c("06-lightsheet-rot-fused222-lz4", "lightsheet", True, False, "fused", (2, 2, 2), LZ4, True, True, True, "both", entry=True),
    _c("07-lightsheet-fused122-runs-2ranks", "lightsheet", False, False, "fused", (1, 2, 2), "blosc", "runs", False, False, "output", ranks=2),
    _c("08-stripes-rot-fused222-2ranks", "stripes", True, False, "fused", (2, 2, 2), "blosc", True, True, True, "both", ranks=2),
    _c("09-lightsheet-rot-host-path-zlib", "lightsheet", True, False, None, None, "zlib", False, False, True, "both", retile=False),
    _c("10-march-pipelined222-2ranks", "streaks:march", False, False, "pipelined", (2, 2, 2), "blosc", True, True, False, "both", ranks=2),
    _c("11-generic-rot-shaded-fused212-runs", "streaks:generic", True, True, "fused", (2, 1, 2), "blosc", "runs", "full", False, "output"),
    _c("12-lightsheet-pipelined212", "lightsheet", False, False, "pipelined", (2, 1, 2), "blosc", True, "any", True, "output"),
    _c("13-lightsheet-rot-fused221-raw", "lightsheet", True, False, "fused", (2, 2, 1), None, False, "full", False, "both"),
    _c("14-march-fused122-host-codec", "streaks:march", False, True, "fused", (1, 2, 2), LZ4, False, False, True, "both"),
    _c("15-stripes-fused221-lz4-zlib-in", "stripes", False, False, "fused", (2, 2, 1), LZ4, True, "full", False, "output"),
    _c("16-stripes-one-level-raw-2ranks", "stripes", False, True, None, None, None, False, False, True, "output", ranks=2),
    _c("17-generic-host-path", "streaks:generic", False, False, None, None, "blosc", False, False, False, "output", retile=False),
    _c("18-lightsheet-rot-pipelined122-raw-2ranks", "lightsheet", True, False, "pipelined", (1, 2, 2), None, False, False, True, "output", ranks=2),
]  # fmt: skip
BY_NAME = {c.name: c for c in CASES}

# the options of the pairwise cover and their values; ``route`` and ``shading`` apply to some filters only
OPTIONS = {
    "route": ("march", "generic"),
    "shading": (False, True),
    "pyramid": (None, "fused", "pipelined"),
    "scale": ((2, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 1)),
    "codec": ("off", "literals", "runs", "lz4"),  # the device encoder's mode: True is "lz4" on a Blosc-LZ4 output
    "decode": (False, True, "any", "full"),
    "hist": (False, True),
    "proj": ("output", "both"),
    "ranks": (1, 2),
}
# the output compressors and the host path are held to both values of ``rotate``, not to every filter
ROTATE_ONLY = {"out": ("blosc", "lz4", "zlib", None), "retile": (True, False)}


def applies(option, filt):
    return {"route": filt == "streaks", "shading": filt != "lightsheet"}.get(option, True)


def codec_mode(case):
    """What ``LAST_RUN["device_codec_mode"]`` must say."""
    if not case.codec:
        return None
    return "runs" if case.codec == "runs" else "lz4" if isinstance(case.out, dict) else "literals"


def _value(case, option):
    if option == "codec":
        return codec_mode(case) or "off"
    v = getattr(case, option)
    return "lz4" if isinstance(v, dict) else v


def uncovered_pairs(cases=None):
    """``(option, value, "filter" / "rotate", its value)`` of every pair the case list does not hold."""
    cases = CASES if cases is None else cases
    missing = []
    for option, values in itertools.chain(OPTIONS.items(), ROTATE_ONLY.items()):
        for v in values:
            have = [c for c in cases if _value(c, option) == v]
            if option in OPTIONS:
                for f in ("stripes", "streaks", "lightsheet"):
                    if applies(option, f) and not any(c.filter == f for c in have):
                        missing.append((option, v, "filter", f))
            for r in (False, True):
                if not any(c.rotate is r for c in have):
                    missing.append((option, v, "rotate", r))
    for f in ("stripes", "streaks", "lightsheet"):
        for r in (False, True):
            if not any(c.filter == f and c.rotate is r for c in cases):
                missing.append(("filter", f, "rotate", r))
    return missing


# ---- input --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volume(seed=SEED):
    """The planes as they are written to the input store (frozen)."""
    vol = synth.synthetic_stack(Z, H, W).astype(np.int64)
    rng = np.random.default_rng(seed)
    ramp = 0.5 + 0.5 * np.cos(np.arange(W)[None, :] / W * 3.0)
    for z in range(Z):  # the row glow of lightsheet_cases.glow_plane, below the foreground cut of the config decision
        rows = rng.integers(0, GLOW, size=(H, 1)) * (rng.random((H, 1)) < 0.3)
        vol[z] += (rows * ramp).astype(np.int64)
    vol = np.clip(vol, 0, 65535).astype(np.uint16)
    vol.setflags(write=False)
    return vol


def missing_region():
    """The (z, y, x) slices of the volume the deleted input chunk covers."""
    return tuple(slice(i * c, min((i + 1) * c, n)) for i, c, n in zip(MISSING, IN_CHUNKS[-3:], (Z, H, W)))


@functools.lru_cache(maxsize=None)
def effective_volume(seed=SEED):
    """What a reader of the input store sees: :func:`volume` with ``FILL_VALUE`` where the chunk file is missing."""
    vol = volume(seed).copy()
    vol[missing_region()] = FILL_VALUE
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def shading():
    """``(flat float32 [H, W], dark float32 [H + 10, W + 6])``: a dark larger than the plane, integer-valued so that the
    uint16 TIFF of a derivatives folder holds the same plane."""
    yy, xx = np.mgrid[0:H, 0:W]
    flat = (1.0 - 0.2 * ((yy / H - 0.4) ** 2 + (xx / W - 0.6) ** 2)).astype(np.float32)
    dark = (90 + np.arange((H + 10) * (W + 6)).reshape(H + 10, W + 6) % 17).astype(np.float32)
    flat.setflags(write=False)
    dark.setflags(write=False)
    return flat, dark


@functools.lru_cache(maxsize=None)
def _shadow_correction():
    flat, dark = shading()
    return {"retrospective": True, "flatfield": flat, "darkfield": dark}


def shadow_correction(case):
    return _shadow_correction() if case.shading else None


def in_compressor(case):
    return {"any": LZ4, "full": "zlib"}.get(case.decode, "blosc")


def block_z(case):
    return 4 if case.pyramid == "fused" and case.scale[0] == 1 else BLOCK_Z


def streaks_dict(case):
    if case.filter != "streaks":
        return None
    return dict(STREAKS[case.route], **({"shading": True} if case.shading else {}))


def store_kwargs(case):
    """The filter options of ``destripe_zarr_store`` / ``destripe_zarr`` for a case."""
    return dict(streaks=streaks_dict(case), lightsheet=dict(LIGHTSHEET) if case.filter == "lightsheet" else None,
                rotate=case.rotate)  # fmt: skip


# ---- geometry, stated without the planner ---------------------------------------------------------------------------------
def level_geometry(scale, n_levels):
    """``[(shape, chunks)]`` of the levels 1 .. n_levels - 1: ``previous // factor`` per axis, the chunk clamped."""
    out, cur = [], (Z, H, W)
    for _ in range(1, n_levels):
        cur = tuple(n // f for n, f in zip(cur, scale))
        out.append((cur, tuple(min(c, n) for c, n in zip(OUT_CHUNKS[-3:], cur))))
    return out


def rank_ranges(case):
    """z range per rank: whole output z chunks spread evenly; with the fused pyramid whole chunk rows of its last level."""
    unit = OUT_CHUNKS[-3]
    if case.pyramid == "fused":
        unit *= case.scale[0] ** (case.n_levels - 1)
    n = -(-Z // unit)
    out, first = [], 0
    for r in range(case.ranks):
        count = n // case.ranks + (1 if r < n % case.ranks else 0)
        out.append((min(first * unit, Z), min((first + count) * unit, Z)))
        first += count
    return out


def z_blocks(case, z_range):
    bz = block_z(case)
    return [(z, min(z + bz, z_range[1])) for z in range(z_range[0], z_range[1], bz)]


def expected_decode_routes(case, z_range):
    """``(chunk reads, of them missing)`` of the device path over a rank's range: a block reads every input chunk its
    planes touch, so a chunk that two blocks share is read, and counted, twice."""
    cz, cy, cx = IN_CHUNKS[-3:]
    reads = fill = 0
    for z0, z1 in z_blocks(case, z_range):
        zs = range(z0 // cz, -(-z1 // cz))
        reads += len(zs) * -(-H // cy) * -(-W // cx)
        fill += sum(1 for z in zs if z == MISSING[0])
    return reads, fill


# ---- level 0 --------------------------------------------------------------------------------------------------------------
def exact_level0(case, vol=None):
    """(device) The per-plane API of the case's filter over the whole volume in uint16."""
    from aind_smartspim_destripe_amd import filtering as fl

    vol = effective_volume() if vol is None else vol
    if case.filter == "lightsheet":
        return fl.correct_lightsheet_planes(vol, rotate=case.rotate, out_dtype=np.uint16, **LIGHTSHEET)
    flat, dark = shading() if case.shading else (None, None)
    if case.filter == "streaks":
        kw = {k: v for k, v in STREAKS[case.route].items() if k != "sigma"}
        return fl.destripe_streaks_planes(vol, SIGMA, out_dtype=np.uint16, flat=flat, dark=dark, rotate=case.rotate, **kw)
    return fl.destripe_planes(vol, TILE, NO_CELLS, CELLS, shadow_correction(case), HIGH_INT, out_dtype=np.uint16,
                              rotate=case.rotate)  # fmt: skip


def exact_key(case):
    return (case.filter, case.route, case.rotate, case.shading)


def _turned(a, k=1):
    return None if a is None else np.ascontiguousarray(np.rot90(a, k))


def stripes_reference(plane, rotate, shaded):
    """``orc.filter_stripes`` of one plane (any dtype regime) as the store holds it: uint16, ``rotate`` as
    ``np.rot90(ref(np.rot90(x)), -1)`` with the shading planes cropped to the plane and turned with it."""
    sc = None
    if shaded:
        flat, dark = shading()
        dark = dark[:H, :W]
        sc = {"retrospective": True, "flatfield": _turned(flat) if rotate else flat, "darkfield": _turned(dark) if rotate else dark}
    ref = orc.filter_stripes(_turned(plane) if rotate else plane, TILE, NO_CELLS, CELLS, sc, HIGH_INT)
    ref = np.clip(ref, 0, 65535).astype(np.uint16)
    return _turned(ref, -1) if rotate else ref


def independent_plane(case, plane):
    """``(reference uint16 [H, W], counts allowed)`` of one input plane from the NumPy references of the suite."""
    if case.filter == "stripes":
        return stripes_reference(plane, case.rotate, case.shading), 1
    x = _turned(plane) if case.rotate else plane
    if case.filter == "lightsheet":
        ref = lc.lightsheet_numpy(x, **LIGHTSHEET)[0]
        tol = 0
    else:
        flat, dark = shading() if case.shading else (None, None)
        if flat is not None and case.rotate:
            flat, dark = _turned(flat), _turned(dark[:H, :W])
        kw = {k: v for k, v in STREAKS[case.route].items() if k not in ("sigma", "route")}
        _, ref = soo.filter_streaks(x, SIGMA, flat=flat, dark=dark, **kw)
        assert ref.max() < 9000  # 1e-4 (1 + v) stays below one count
        tol = 1
    ref = np.clip(ref, 0, 65535).astype(np.uint16)
    return (_turned(ref, -1) if case.rotate else ref), tol


# ---- what follows from level 0 ----------------------------------------------------------------------------------------------
def expected_levels(level0, case):
    """Levels 1 .. of the store's own level 0: the windowed mean of the previous level, truncated."""
    if not case.pyramid:
        return []
    return fo.pyramid(level0, case.n_levels, case.scale)[1:]


def expected_bricks(level_volume, chunks):
    """``{(bz, by, bx): brick}`` of a level: every chunk file whole, fill value 0 outside the array."""
    bricks = fo.planes_to_bricks(level_volume, chunks)
    return {idx: bricks[idx] for idx in itertools.product(*(range(n) for n in bricks.shape[:3]))}


def expected_histogram(level0):
    return np.bincount(level0.ravel(), minlength=65536).astype(np.int64)


def expected_window(level0):
    lo, hi = (float(v) for v in np.percentile(level0, (0.1, 95), method="lower"))
    return lo, max(hi, lo + 1.0)


def expected_scales(case):
    """The ``scale`` transform of every level of the group's metadata."""
    f = case.scale or (2, 2, 2)
    return [[1.0, 1.0] + [v * k**lvl for v, k in zip((XYZ[2], XYZ[1], XYZ[0]), f)] for lvl in range(case.n_levels)]


# ---- the input store ----------------------------------------------------------------------------------------------------------
def write_input(folder, compressor):
    """``<folder>/X_0_Y_0.zarr/0``: :func:`volume` in ``IN_CHUNKS`` with ``FILL_VALUE``, the chunk ``MISSING`` deleted.
    Returns the tile path."""
    tile = os.path.join(str(folder), TILE + ".zarr")
    src = MiniZarrArray.create(os.path.join(tile, "0"), (1, 1, Z, H, W), IN_CHUNKS, np.uint16, compressor=compressor,
                               fill_value=FILL_VALUE)  # fmt: skip
    src[0, 0] = volume()
    os.remove(src._chunk_path((0, 0) + MISSING))
    return tile
