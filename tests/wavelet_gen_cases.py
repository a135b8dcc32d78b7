"""Cases of the tap-count-generic wavelet level kernels (``csrc/dsx_wavelet.h``: ``k_fwd_gen``, ``k_inv_gen``), shared by
the CPU test (``test_wavelet_gen_cases_host.py``) and the GPU tests (``test_gpu_wavelet_gen.py``).  NumPy only.

``cases()`` returns the same list in the same order every time: ``(name, wavelet, planes, level, sigma,
max_threshold)``, ``wavelet`` a PyWavelets name or an object with ``dec_lo ... rec_hi``, ``planes`` uint16 or float32
``[n, H, W]`` from ``synth.synthetic_plane`` / ``synthetic_bank``, no plane above 420 x 420.

What the shapes are for.  ``k_fwd_gen`` gives a block 16 x 32 coefficients and pulls a ``(30 + F) x (62 + F)`` patch
through ``4 (62 + F)(63 + F)`` bytes of dynamic LDS; ``k_inv_gen`` gives a block 32 x 64 results (the plane at the last
level, ``c_{l-1}`` -- the shape of the level below -- at a pyramid level); level shapes follow ``(n + F - 1) // 2``.

* ``lds_under`` / ``lds_over``  db32 (64 taps, 64 008 B) and db33 (66 taps, 66 048 B) on the same 140 x 201 plane, one
  level: the last bank that runs under the default 64 KiB of dynamic LDS and the first that needs the raised limit.
* ``longest``   coif17 (102 taps, 108 240 B), 407 x 412, two levels (254 x 256, then 177 x 178): the longest bank of the
  table, 16 x 8 and 12 x 6 blocks forward, an odd plane (one replicated result row).
* ``capacity``  coif17 with one zero tap at each end (104 taps = ``kMaxTaps``), handed over as an object, 150 x 131.
* ``wrap_coif17`` 24 x 30 at level 2 (62 x 65, then 81 x 83) and ``wrap_db11`` 41 x 47 at level 4: planes shorter than
  the filter, so the symmetric extension reflects several times and the levels GROW (the reference warns and runs).
* ``tile_edges_<bank>_<on|past|short>``  db38 (76 taps) and sym4 (8 taps), two levels: level-1 shapes ``(16 a, 32 b)``,
  ``(16 a + 1, 32 b + 1)``, ``(16 a - 1, 32 b - 1)`` -- coefficient tiles that end exactly on, one past and one short of
  the level -- with ``b`` even and ``a`` even, so that the level-2 synthesis, which writes ``c_1`` of that shape in
  tiles of 32 x 64, meets ``w % 64`` in {0, 1, 63} and ``h % 32`` in {0, 1, 31} too.  ``tile_residues()`` returns the
  residues and the module asserts them at import.
* ``short``     haar (2 taps), 33 x 65, full depth: five levels down to 2 x 3.
* ``deep``      db16 (32 taps), 251 x 300, full depth: three levels with a mid-length bank.
* ``batch_u16`` / ``batch_f32``  db33, five planes 131 x 203; planes 0 and 4 carry cells, so a run with the config pair
  of ``configs()`` takes both configs; uint16 and float32 input.
* ``bior39`` / ``rbio39``  20 taps, ``rec`` is not the reversed ``dec`` and the L1 norms of the four filters differ.
* ``saturate``  db4, a float32 plane with cells scaled by 20: results beyond 65 535 for the uint16 cast.

The taps of sym4 as PyWavelets prints them miss perfect reconstruction by 1e-12 (every other bank here by 1e-16), so the
sym4 planes carry no cells (log values up to 5.6): their float64 round trip then stays inside the 1e-12 the host test
asks of every bank.

Left out on purpose: an odd plane where one config has levels and the other has none (a documented limit), and
``rbio3.1`` (its own test and bound, ``tests/test_wavelets.py``)."""

import numpy as np

from aind_smartspim_destripe_amd import synth, wavelets

HIGH_INT = synth.ZARR_PATH_HIGH_INT
MAX_PLANE = 420
LDS_DEFAULT = 64 * 1024  # dynamic LDS a kernel may ask for without hipFuncSetAttribute
FWD_TILE, INV_TILE = (16, 32), (32, 64)  # kGenTH x kGenTW, kGenOH x kGenOW (csrc/dsx_chain.h)


class Bank:
    """A filter bank as an object with the four attributes of a ``pywt.Wavelet``."""

    def __init__(self, name, dec_lo, dec_hi, rec_lo, rec_hi):
        self.name = name
        self.dec_lo, self.dec_hi, self.rec_lo, self.rec_hi = (np.asarray(f, np.float64) for f in (dec_lo, dec_hi, rec_lo, rec_hi))


def padded_bank(name, pad=1):
    """``name`` with ``pad`` zero taps at each end of every filter.  Two zero taps more shift analysis and synthesis by
    one sample each way, so the longer bank is a perfect-reconstruction bank again (the host test checks the round
    trip)."""
    return Bank("%s+%d" % (name, 2 * pad), *[np.pad(f, pad) for f in wavelets.filter_bank(name)])


def bank_of(wavelet):
    """``(dec_lo, dec_hi, rec_lo, rec_hi)`` float64 of a case's wavelet, what the oracle takes."""
    return wavelets.filter_bank(wavelet)


def taps(wavelet):
    return len(bank_of(wavelet)[0])


def gen_fwd_lds_bytes(F):
    """``gen_fwd_lds_bytes`` of ``csrc/dsx_chain.h`` in closed form."""
    return 4 * (62 + F) * (63 + F)


def level_shapes(shape, F, levels):
    """Coefficient shapes of levels 1 .. ``levels``: ``(n + F - 1) // 2`` per axis and level."""
    out, (h, w) = [], shape
    for _ in range(levels):
        h, w = (h + F - 1) // 2, (w + F - 1) // 2
        out.append((h, w))
    return out


# name suffix -> plane shape per bank: the level-1 shape is (16 a, 32 b) + (0 | +1 | -1) with a = 6, b = 4 (db38) and
# a = 2, b = 2 (sym4); heights and widths of both parities
_TILE_EDGE_SHAPES = {
    "db38": {"on": (118, 181), "past": (119, 184), "short": (115, 180)},
    "sym4": {"on": (58, 121), "past": (59, 124), "short": (55, 120)},
}


def tile_residues():
    """Per bank of the ``tile_edges`` cases, in the order on / past / short: ``(h % 16, w % 32, h % 32, w % 64)`` of the
    level-1 shape ``(h, w)``."""
    out = {}
    for name, shapes in _TILE_EDGE_SHAPES.items():
        F = taps(name)
        res = []
        for key in ("on", "past", "short"):
            h, w = level_shapes(shapes[key], F, 1)[0]
            assert h >= 2 * FWD_TILE[0] - 1 and w >= 2 * FWD_TILE[1] - 1  # a, b >= 2
            res.append((h % FWD_TILE[0], w % FWD_TILE[1], h % INV_TILE[0], w % INV_TILE[1]))
        out[name] = res
    return out


for _res in tile_residues().values():
    assert _res == [(0, 0, 0, 0), (1, 1, 1, 1), (15, 31, 31, 63)], _res


def _plane(k, h, w):
    return synth.synthetic_plane(k, h, w)[None]


def cases():
    c = [
        ("lds_under", "db32", _plane(1, 140, 201), 1, 64, 4),
        ("lds_over", "db33", _plane(1, 140, 201), 1, 64, 4),
        ("longest", "coif17", _plane(2, 407, 412), 2, 128, 12),
        ("capacity", padded_bank("coif17"), _plane(3, 150, 131), 1, 64, 4),
        ("wrap_coif17", "coif17", _plane(5, 24, 30), 2, 16, 3),
        ("wrap_db11", "db11", _plane(6, 41, 47), 4, 32, 12),
    ]
    for name, shapes in _TILE_EDGE_SHAPES.items():
        for i, key in enumerate(("on", "past", "short")):
            c.append(("tile_edges_%s_%s" % (name, key), name, _plane(5 + i, *shapes[key]), 2, 64, 4))
    c += [
        ("short", "haar", _plane(10, 33, 65), None, 64, 4),
        ("deep", "db16", _plane(11, 251, 300), None, 128, 12),
        ("batch_u16", "db33", synth.synthetic_bank(5, 131, 203), 1, 128, 12),
        ("batch_f32", "db33", synth.synthetic_bank(5, 131, 203).astype(np.float32), 1, 128, 12),
        ("bior39", "bior3.9", _plane(13, 120, 151), 2, 64, 4),
        ("rbio39", "rbio3.9", _plane(13, 120, 151), 2, 64, 4),
        ("saturate", "db4", _plane(12, 64, 96).astype(np.float32) * np.float32(20.0), 2, 64, 4),
    ]
    for name, _, planes, _, _, _ in c:
        assert planes.ndim == 3 and max(planes.shape[1:]) <= MAX_PLANE, name
    return c


def config(case, oracle=False):
    """The case's own config dict; ``oracle=True``: with the filter bank itself, what the oracle takes."""
    _, wavelet, _, level, sigma, max_threshold = case
    return {"wavelet": bank_of(wavelet) if oracle else wavelet, "level": level, "sigma": sigma, "max_threshold": max_threshold}


def configs(case, oracle=False):
    """``(cells, nocells)`` of a whole-path run: the case's config for planes without cells and, as in production, half
    the sigma and a threshold cap of 3 for planes with cells."""
    nocells = config(case, oracle)
    return dict(nocells, sigma=nocells["sigma"] / 2, max_threshold=3), nocells
