"""Cases of the light-sheet background mode (README "Light-sheet background mode"), shared by the CPU tests
(``test_lightsheet_host.py``), the GPU tests (``test_gpu_lightsheet.py``) and the fixture tool
(``tools/make_golden_lightsheet.py``), and the NumPy restatement of the contract.  NumPy only.

What the shapes are for (``csrc/dsx_lightsheet.h``: ``k_ls_row`` splits a row into runs of 64 output pixels, ``k_ls_bg``
tiles a plane by strips of ``600 - (B - 1)`` columns and segments of 32 rows, four waves share a strip):

* ``border``   37 x 53, A = 150, B = 200: every window is cut by the border, ``n`` varies everywhere.
* ``odd`` / ``even``  64 x 96, (A, B) = (15, 20) and (7, 6): the centre rule of odd and even sizes.
* ``default``  230 x 310, the defaults: the B x B window has an interior; 310 spans five runs of a row.
* ``tiles``    66 x 810, A = 15, B = 201: strips of 400 columns and segments of 32 rows, so the width spans three
  strips (400, 400, 10) and the height three segments (32, 32, 2); a row spans thirteen runs.
* ``one``      A = 1, B = 1: the offset is the plane's own quantised value.
* ``wideA``    5 x 2200, A = 1024: the 16-bit counts of the row filter.  ``bigB`` 256 x 257, B = 255, with a constant
  field larger than the window: one bin of the window histogram reaches 255 * 255 = 65 025.
* ``zeros`` / ``full``  constant planes at 0 and at 65 535.
* ``square``   one bright 40 x 40 square on glow: around it the line estimate exceeds lambda times the regional one and
  the branch takes ``G``.
* ``p10`` / ``p50``  p = 0.1 and 0.5 (0.25 everywhere else).
"""

import numpy as np

DEFAULTS = dict(percentile=0.25, artifact_length=150, background_window_size=200, lightsheet_vs_background=2.0)


def quantise(x):
    """Step 1 in NumPy float64: ``floor(255 log2(1 + x) / 16)`` as uint8."""
    return np.floor(255.0 * np.log2(1.0 + np.asarray(x, np.float64)) / 16.0).astype(np.uint8)


def back_table():
    """``Bk[v] = float32(2 ** (16 v / 255) - 1)``."""
    return (np.exp2(16.0 * np.arange(256, dtype=np.float64) / 255.0) - 1.0).astype(np.float32)


def _inside(size, length):
    """Per position i of an axis of ``size``: first and one-past-last index of the window i - length // 2 ..
    i - length // 2 + length - 1 cut to the axis."""
    first = np.arange(size) - length // 2
    return np.maximum(first, 0), np.minimum(first + length, size)


def percentile_numpy(q, h, w, p):
    """Step 2 restated: per pixel the smallest v with ``#{q <= v in the window} > p * n`` (float64 product), the window
    cut to the plane.  Counts come from one summed-area table per v."""
    H, W = q.shape
    r0, r1 = _inside(H, h)
    c0, c1 = _inside(W, w)
    n = ((r1 - r0)[:, None] * (c1 - c0)[None, :]).astype(np.float64)
    bound = np.float64(p) * n
    out = np.zeros((H, W), np.int64)
    sat = np.zeros((H + 1, W + 1), np.int64)
    for v in range(255):  # (at v = 255 the count is n > p n: nothing left to add)
        sat[1:, 1:] = np.cumsum(np.cumsum(q <= v, axis=0, dtype=np.int64), axis=1)
        count = sat[r1][:, c1] - sat[r0][:, c1] - sat[r1][:, c0] + sat[r0][:, c0]
        out += ~(count > bound)
    return out.astype(np.uint8)


def subtract_numpy(x, ls, bg, lam, back=None):
    """Step 3 restated in float32."""
    back = back_table() if back is None else back
    L, G = back[ls], back[bg]
    offset = np.where(L <= np.float32(lam) * G, L, G)
    return np.maximum(x.astype(np.float32) - offset, np.float32(0))


def lightsheet_numpy(x, percentile=0.25, artifact_length=150, background_window_size=200, lightsheet_vs_background=2.0):
    """The whole contract over one uint16 plane: ``(out float32, q, ls, bg)``."""
    q = quantise(x)
    ls = percentile_numpy(q, 1, artifact_length, percentile)
    bg = percentile_numpy(q, background_window_size, background_window_size, percentile)
    return subtract_numpy(x, ls, bg, lightsheet_vs_background), q, ls, bg


def glow_plane(seed, H, W, square=None):
    """Background of ~200 counts, an additive glow along x that differs from row to row, a few bright blobs, 5 bits of
    noise; ``square = (r, c, size)`` adds one bright square."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 400, size=(H, 1)) * (rng.random((H, 1)) < 0.3)
    ramp = 0.5 + 0.5 * np.cos(np.arange(W)[None, :] / max(W, 2) * 3.0)
    img = 200.0 + rows * ramp + rng.integers(0, 32, size=(H, W))
    for _ in range(3):
        r, c, s = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 9)
        img[max(r - s, 0) : r + s, max(c - s, 0) : c + s] += rng.integers(1000, 20000)
    if square is not None:
        r, c, s = square
        img[r : r + s, c : c + s] += 6000
    return np.clip(img, 0, 65535).astype(np.uint16)


def field_plane(seed, H, W):
    """A constant field (value 300) larger than a 255 x 255 window, noise around it."""
    img = glow_plane(seed, H, W)
    img[:, :] = np.where(np.arange(W)[None, :] < W - 2, 300, img)
    img[0, :] = 7
    return img


def _params(**kw):
    return dict(DEFAULTS, **kw)


def cases():
    """``[(name, plane uint16 [H, W], params dict)]``; the same list, in the same order, every time."""
    return [
        ("border", glow_plane(1, 37, 53), _params()),
        ("odd", glow_plane(2, 64, 96), _params(artifact_length=15, background_window_size=20)),
        ("even", glow_plane(3, 64, 96), _params(artifact_length=7, background_window_size=6)),
        ("default", glow_plane(4, 230, 310), _params()),
        ("tiles", glow_plane(5, 66, 810), _params(artifact_length=15, background_window_size=201)),
        ("one", glow_plane(6, 33, 70), _params(artifact_length=1, background_window_size=1)),
        ("wideA", glow_plane(7, 5, 2200), _params(artifact_length=1024, background_window_size=3)),
        ("bigB", field_plane(8, 256, 257), _params(artifact_length=9, background_window_size=255)),
        ("zeros", np.zeros((40, 50), np.uint16), _params(artifact_length=15, background_window_size=20)),
        ("full", np.full((40, 50), 65535, np.uint16), _params(artifact_length=15, background_window_size=20)),
        ("square", glow_plane(9, 120, 130, square=(40, 45, 40)), _params(artifact_length=100, background_window_size=90)),
        ("p10", glow_plane(10, 64, 96), _params(percentile=0.1, artifact_length=15, background_window_size=20)),
        ("p50", glow_plane(11, 64, 96), _params(percentile=0.5, artifact_length=15, background_window_size=20)),
    ]  # fmt: skip


def case_names():
    return [c[0] for c in cases()]
