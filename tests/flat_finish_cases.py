"""The cases the native finish of a flat (``csrc/dsx_smooth.h``) is held to, shared by ``test_flat_finish_host.py`` (the
host build against NumPy) and ``test_gpu_flat_finish.py`` (the kernels against the host build, bit for bit).

Smoothing cases: the tile lengths come from the geometry function the launch uses (restated here as ``TILES`` and checked
against the library's behaviour by the stand-alone program ``tests/host/flat_finish_check.cpp``): on each axis every tile
length at -1, +0 and +1 and twice the tile plus 1; planes so short that the fold runs several times; ``n = r``, ``r + 1``
and ``2 r + 1`` on each axis; odd widths; every sigma of ``SIGMAS``; non-negative whole counts and signed data; a base
that is 16-byte aligned (the 16-byte load body) and one that is only 8-byte aligned (``lead = 1``: the scalar body).
"""

import collections
import functools

import numpy as np

from aind_smartspim_destripe_amd import engine as eng_mod

SIGMAS = (0, 0.3, 1, 2, 2.25, 32, 64)
# tile lengths of dsx::sm::geometry per axis: k_sm_col owns 32 rows x 32 columns, k_sm_row 16 rows x 64 columns
TILES = {"y": (32, 16), "x": (32, 64)}
MEAN_LANES = 4096

SmoothCase = collections.namedtuple("SmoothCase", "name plane sigma lead")
FinishCase = collections.namedtuple("FinishCase", "name rank valid shape sigma floor")


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def _plane(rs, shape, signed):
    if signed:
        return np.ascontiguousarray(rs.standard_normal(shape) * 3000.0)
    return np.floor(rs.random_sample(shape) * 60000.0)  # whole counts, as a rank plane holds them


def _shapes():
    """``(shape, sigma)`` of every smoothing case."""
    out = []
    # planes the fold crosses several times
    for shape in ((1, 1), (1, 37), (37, 1), (2, 3), (3, 5)):
        for sigma in (2, 2.25, 32):
            out.append((shape, sigma))
    out.append(((2, 3), 64))
    # n = r, r + 1, 2 r + 1 on each axis
    for sigma in (2, 2.25, 32):
        r = radius(sigma)
        out += [((r, r + 1), sigma), ((r + 1, 2 * r + 1), sigma), ((2 * r + 1, r), sigma)]
    out += [((256, 40), 64), ((40, 256), 64), ((257, 24), 64), ((40, 257), 64), ((513, 24), 64), ((24, 513), 64)]
    # tile lengths at -1, +0, +1 and twice the tile plus 1, on each axis, every sigma in turn
    ys = [t + d for t in TILES["y"] for d in (-1, 0, 1)] + [2 * t + 1 for t in TILES["y"]]
    xs = [t + d for t in TILES["x"] for d in (-1, 0, 1)] + [2 * t + 1 for t in TILES["x"]]
    for i, (h, w) in enumerate(zip(ys, xs)):
        out.append(((h, w), SIGMAS[i % len(SIGMAS)]))
        out.append(((ys[-1 - i], w), SIGMAS[(i + 3) % len(SIGMAS)]))
    # every sigma on one plane of several tiles each way, odd and even width
    for sigma in SIGMAS:
        out.append(((45, 131), sigma))
    out += [((70, 130), 1), ((70, 130), 32), ((300, 520), 64), ((299, 519), 32)]
    return out


@functools.lru_cache(maxsize=None)
def smooth_cases():
    rs = np.random.RandomState(77)
    cases = []
    for i, (shape, sigma) in enumerate(_shapes()):
        signed, lead = bool(i & 1), int((i >> 1) & 1)
        name = "{}x{}_s{}_{}{}".format(shape[0], shape[1], sigma, "signed" if signed else "counts", "_lead" if lead else "")
        cases.append(SmoothCase(name, _plane(rs, shape, signed), float(sigma), lead))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def smooth_ids():
    return [c.name for c in smooth_cases()]


@functools.lru_cache(maxsize=None)
def smooth_reference():
    """The host build's result of every smoothing case, computed once: ``{name: float64 plane}``."""
    return {c.name: eng_mod.gauss_smooth_ref(c.plane, eng_mod.gauss_taps(c.sigma)[1]) for c in smooth_cases()}


def _field(rs, n_q, Hs, Ws, level, spread):
    y, x = np.mgrid[0:Hs, 0:Ws]
    base = level * (1.0 - 0.3 * ((y / max(Hs - 1, 1) - 0.5) ** 2 + (x / max(Ws - 1, 1) - 0.5) ** 2))
    planes = [np.clip(base / (1 + 3 * q) + rs.randint(-spread, spread + 1, (Hs, Ws)), 0, 65535) for q in range(n_q)]
    return np.stack(planes).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def finish_cases():
    rs = np.random.RandomState(78)
    cases = []

    def add(name, rank, valid, shape, sigma, floor=0.1):
        cases.append(FinishCase(name, np.ascontiguousarray(rank), np.ascontiguousarray(valid.astype(np.uint16)), shape, float(sigma), floor))

    # everything seen, one and two rank planes, several tiles, odd width
    rank = _field(rs, 2, 45, 131, 900, 40)
    add("seen_all_nq1", rank[:1], np.full((45, 131), 7), (45, 131), 2.25)
    add("seen_all_nq2", rank, np.full((45, 131), 7), (45, 131), 2.25)
    # an unseen block and scattered unseen pixels
    valid = rs.randint(0, 5, (45, 131))
    valid[10:30, 50:100] = 0
    add("unseen_region_nq2", rank, valid, (45, 131), 2)
    # an even seen count whose two middle values differ by an odd number: the fill ends in .5
    rank = np.array([[[10, 13, 500, 20, 700, 11]]], np.uint16).repeat(2, axis=0)
    valid = np.array([[1, 1, 0, 1, 0, 1]])
    add("even_count_half", rank, valid, (1, 6), 1)
    # stored planes larger than the image (odd planes grown to even): the crop, with other values outside it
    rank = _field(rs, 2, 32, 48, 2000, 100)
    valid = rs.randint(0, 3, (32, 48))
    rank[:, 31, :] = 65535
    rank[:, :, 47] = 65535
    valid[31, :] = 9
    valid[:, 47] = 9
    add("cropped_31x47", rank, valid, (31, 47), 1)
    # values above the LDS window of the histogram kernel, and across it
    rank = _field(rs, 2, 40, 70, 40000, 3000)
    valid = rs.randint(0, 2, (40, 70))
    add("high_values", rank, valid, (40, 70), 2, 0.9)
    # one value all over (a wave's counted lanes hold one value), with holes
    rank = np.full((1, 33, 64), 321, np.uint16)
    valid = rs.randint(0, 4, (33, 64))
    add("one_value", rank, valid, (33, 64), 0.3)
    # more pixels than one sweep of the histogram's grid and more than the 4096 lanes of the mean hold once
    rank = _field(rs, 2, 300, 520, 1500, 60)
    valid = (rs.random_sample((300, 520)) > 0.02) * 5
    add("large_nq2", rank, valid, (299, 519), 32)
    add("sigma0_nq2", rank[:, :70, :130], valid[:70, :130], (70, 130), 0)
    add("single_pixel", np.array([[[7]]], np.uint16), np.array([[1]]), (1, 1), 2)
    add("single_seen_of_many", _field(rs, 1, 5, 9, 100, 3), np.eye(5, 9), (5, 9), 64)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def finish_ids():
    return [c.name for c in finish_cases()]


@functools.lru_cache(maxsize=None)
def finish_reference():
    """The host build's ``(flat, dark)`` of every finish case, computed once."""
    return {c.name: eng_mod.flat_finish_ref(c.rank, c.valid, c.shape, eng_mod.gauss_taps(c.sigma)[1], c.floor)
            for c in finish_cases()}  # fmt: skip


def numpy_finish(case):
    """Steps 2 to 4 of ``estimate_fields`` in NumPy (today's finish) on the crop of a finish case: ``(flat, dark)``."""
    from aind_smartspim_destripe_amd import flatfield_estimation as fe

    H, W = case.shape
    seen = case.valid[:H, :W] > 0
    planes = []
    for r in case.rank[:, :H, :W]:
        r = r.astype(np.float64)
        if not seen.all():
            r[~seen] = np.median(r[seen])
        planes.append(fe.gaussian_smooth(r, case.sigma))
    flat = np.maximum(planes[0] / planes[0].mean(), case.floor).astype(np.float32)
    return flat, (planes[1].astype(np.float32) if len(planes) > 1 else None)
