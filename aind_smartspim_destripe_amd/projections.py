"""QC projections of a store pass: the three maximum-intensity projections of a uint16 volume and its three sum
projections, collected while the planes of a block lie in device memory (``csrc/dsx_project.h``), merged over the ranks
and written where a person can look at them.

Stripes are constant along x, so the sum of every row before the filter and after it is the stripe signature and what
became of it; their ratio is the gain the filter applied to that row -- one small ``[Z, H]`` image per tile that shows
missed stripes, planes that took the wrong config and structure that was flattened (:func:`stripe_gain`).

For ``v[Z, H, W]`` (``engine.PROJECTION_ARRAYS``): ``max_z`` / ``sum_z`` ``[H, W]`` uint16 / uint64, ``max_y`` / ``sum_y``
``[Z, W]`` uint16 / uint32, ``max_x`` / ``sum_x`` ``[Z, H]`` uint16 / uint32.  Every array starts as zeros, the identity
of both reducers on uint16 data, so the projection of a volume is the element-wise max of the max arrays and sum of the
sum arrays of any split of it into z ranges: blocks and ranks add up exactly.
"""

import os

import numpy as np

from . import engine as engine_mod
from . import mini_tiff

NAMES = tuple(name for name, _, _ in engine_mod.PROJECTION_ARRAYS)


def project_volume(v):
    """The six projections of a uint16 ``[Z, H, W]`` array in NumPy: ``{name: array}``."""
    v = np.asarray(v)
    if v.dtype != np.uint16 or v.ndim != 3:
        raise ValueError("project_volume takes a uint16 [Z, H, W] array, got {} {}".format(v.dtype, v.shape))
    if v.shape[0] == 0:
        return {name: np.zeros(shape, dtype) for name, shape, dtype in engine_mod.projection_shapes(v.shape)}
    return {"max_z": v.max(0), "sum_z": v.sum(0, dtype=np.uint64), "max_y": v.max(1), "sum_y": v.sum(1, dtype=np.uint32),
            "max_x": v.max(2), "sum_x": v.sum(2, dtype=np.uint32)}  # fmt: skip


class VolumeProjections:
    """The six projections of a ``zyx`` volume, zeroed, and which planes have been added (``added``, one bool each)."""

    def __init__(self, zyx):
        Z, H, W = (int(n) for n in zyx)
        if Z <= 0 or H <= 0 or W <= 0 or max(H, W) > engine_mod.PROJECT_MAX_EXTENT:
            raise ValueError("projections: a volume of {!r} (at most {} rows and columns)".format(tuple(zyx), engine_mod.PROJECT_MAX_EXTENT))
        self.zyx = (Z, H, W)
        self.arrays = {name: np.zeros(shape, dtype) for name, shape, dtype in engine_mod.projection_shapes(self.zyx)}
        self.added = np.zeros(Z, bool)

    def __getattr__(self, name):
        if name in NAMES:
            return self.__dict__["arrays"][name]
        raise AttributeError(name)

    def _claim(self, z0, n):
        z0, n = int(z0), int(n)
        if z0 < 0 or n < 0 or z0 + n > self.zyx[0]:
            raise ValueError("projections: planes [{}, {}) do not fit a volume of {} planes".format(z0, z0 + n, self.zyx[0]))
        if self.added[z0 : z0 + n].any():
            raise ValueError("projections: plane {} was added before".format(z0 + int(np.argmax(self.added[z0 : z0 + n]))))
        return z0, n

    def add(self, z0, block):
        """Planes ``z0 .. z0 + len(block) - 1`` of the volume: a uint16 ``[n, H, W]`` array (the host build,
        ``engine.project_ref``).  ``ValueError`` for a shape that does not fit and for a plane that was added before."""
        block = np.asarray(block)
        if block.dtype != np.uint16 or block.ndim != 3 or block.shape[1:] != self.zyx[1:]:
            raise ValueError("projections: a block is uint16 [n, {}, {}], not {} {}".format(*self.zyx[1:], block.dtype, block.shape))
        z0, n = self._claim(z0, block.shape[0])
        for z in range(z0, z0 + n, engine_mod.PROJECT_MAX_EXTENT):  # (one call takes 65 536 planes)
            part = block[z - z0 : z - z0 + engine_mod.PROJECT_MAX_EXTENT]
            engine_mod.project_ref(part, acc=self.arrays, z_off=z)
        self.added[z0 : z0 + n] = True

    def add_projected(self, z0, arrays):
        """Planes ``z0 .. z0 + n - 1`` that were projected elsewhere (the device arrays of a rank's z range,
        ``DestripeEngine.project``): ``arrays`` holds the six arrays of those ``n`` planes alone."""
        n = int(np.asarray(arrays["max_y"]).shape[0])
        for name, shape, dtype in engine_mod.projection_shapes((n,) + self.zyx[1:]):
            a = arrays[name]
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape):
                raise ValueError("projections: {} of {} planes is {} {}".format(name, n, dtype, shape))
        z0, n = self._claim(z0, n)
        for name in NAMES:
            if name.endswith("_z"):
                _fold(self.arrays[name], arrays[name], "max" if name.startswith("max") else "sum")
            else:
                self.arrays[name][z0 : z0 + n] = arrays[name]
        self.added[z0 : z0 + n] = True

    def merge(self, group=None):
        """Every rank's planes on every rank: ``group.reduce_array`` per array (max of the max arrays, sum of the sum
        arrays, through the rendezvous directory -- some tens of MB per rank, once per tile); without a group, or with
        one rank, nothing travels.  Afterwards every plane must have been added exactly once, by one rank:
        ``RuntimeError`` on rank 0 otherwise (a missing or doubled plane would falsify the sums), as the voxel count
        of the histogram is checked."""
        count = self.added.astype(np.uint8)
        if group is not None and getattr(group, "active", True) and hasattr(group, "reduce_array"):
            for name in NAMES:
                self.arrays[name] = group.reduce_array(self.arrays[name], "max" if name.startswith("max") else "sum")
            count = group.reduce_array(count, "sum")
        rank = int(getattr(group, "rank", 0)) if group is not None else 0
        if rank == 0 and not (count == 1).all():
            bad = int(np.flatnonzero(count != 1)[0])
            raise RuntimeError("projections: plane {} was added {} times over the ranks ({} of {} planes are wrong)"
                               .format(bad, int(count[bad]), int((count != 1).sum()), count.size))  # fmt: skip
        self.added = count == 1
        return self

    def save(self, path):
        """The six arrays, ``added`` and ``zyx`` as one ``.npz``."""
        np.savez(path, zyx=np.asarray(self.zyx, np.int64), added=self.added, **self.arrays)

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            p = cls(tuple(int(n) for n in f["zyx"]))
            for name, shape, dtype in engine_mod.projection_shapes(p.zyx):
                a = f[name]
                if a.shape != shape or a.dtype != dtype:
                    raise ValueError("{}: {} is {} {}, not {} {}".format(path, name, a.dtype, a.shape, dtype, shape))
                p.arrays[name] = np.ascontiguousarray(a)
            p.added = f["added"].astype(bool)
        return p


def _fold(acc, other, op):
    if op == "max":
        np.maximum(acc, other, out=acc)
    else:
        acc += other


def stripe_gain(inp, out, rotate=False):
    """The gain the filter applied to every row: ``sum_x`` of the output over ``sum_x`` of the input, float32 ``[Z, H]``,
    1.0 where the input row is all zero.  ``rotate=True`` (stripes down the columns): the same of ``sum_y``, ``[Z, W]``."""
    name = "sum_y" if rotate else "sum_x"
    a, b = getattr(inp, name), getattr(out, name)
    if inp.zyx != out.zyx:
        raise ValueError("stripe_gain: the projections are of two volumes ({} and {})".format(inp.zyx, out.zyx))
    gain = np.ones(a.shape, np.float32)
    np.divide(b.astype(np.float32), a.astype(np.float32), out=gain, where=a != 0)
    return gain


def write_qc(folder, name, out, inp=None, rotate=False):
    """What a person looks at after a pass, in ``folder``: ``<name>_projections.npz`` (the six arrays of the output under
    their names; with ``inp`` those of the input with the prefix ``in_`` and ``stripe_gain``) and the 16-bit maxima of
    the output as ``<name>_mip_z.tif`` ``[H, W]``, ``<name>_mip_y.tif`` ``[Z, W]`` and ``<name>_mip_x.tif`` ``[Z, H]``.
    Returns the paths written."""
    os.makedirs(str(folder), exist_ok=True)
    arrays = dict(out.arrays)
    if inp is not None:
        arrays.update({"in_" + k: v for k, v in inp.arrays.items()})
        arrays["stripe_gain"] = stripe_gain(inp, out, rotate=rotate)
    paths = [os.path.join(str(folder), "{}_projections.npz".format(name))]
    np.savez(paths[0], **arrays)
    for axis in "zyx":
        paths.append(os.path.join(str(folder), "{}_mip_{}.tif".format(name, axis)))
        mini_tiff.imwrite(paths[-1], out.arrays["max_" + axis])
    return paths


QC_MODES = (None, "output", "both")


def check_qc_mode(qc_projections):
    """``qc_projections`` of the entry points: ``None``, ``"output"`` or ``"both"``; ``ValueError`` otherwise."""
    if qc_projections is not None and not (isinstance(qc_projections, str) and qc_projections in QC_MODES):
        raise ValueError("qc_projections is None, \"output\" or \"both\", not {!r}".format(qc_projections))
    return qc_projections


def check_store_option(projections, zyx=None):
    """The ``projections`` dict of ``destripe_zarr_store``: ``{"output": VolumeProjections}``, optionally with
    ``"input"``; with ``zyx`` the volumes must have that shape.  Returns ``None``, ``"output"`` or ``"both"``."""
    if projections is None:
        return None
    if not isinstance(projections, dict) or "output" not in projections or set(projections) - {"output", "input"}:
        raise ValueError("projections is a dict with the key \"output\" and optionally \"input\", not {!r}".format(projections))
    for key, p in projections.items():
        if not isinstance(p, VolumeProjections):
            raise ValueError("projections[{!r}] must be a VolumeProjections, not {}".format(key, type(p).__name__))
        if zyx is not None and p.zyx != tuple(int(n) for n in zyx):
            raise ValueError("projections[{!r}] is of a volume {}, the array is {}".format(key, p.zyx, tuple(zyx)))
    return "both" if "input" in projections else "output"
