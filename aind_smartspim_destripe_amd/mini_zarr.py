"""Minimal Zarr-v2 directory store (read / write) for the chunk map.

Neither ``zarr`` nor ``numcodecs`` is installed in this environment, so the chunk map carries its own small
implementation of the subset it needs: C-order arrays, little-endian numeric dtypes, ``compressor`` ``null``,
``zlib`` or ``blosc``, ``"."`` or ``"/"`` chunk-key separators, basic slicing with unit steps.  The reference's
production arrays are ``uint16``, chunks ``(1, 1, 64, 128, 128)``, ``Blosc(cname="zstd", clevel=3, shuffle=SHUFFLE)``,
``dimension_separator="/"`` (``zarr_destriper.py:1066-1074``).  Blosc frames are decoded / encoded by the native
library (``csrc/dsx_io.h``: the c-blosc 1.x container restated from its format description, ``libzstd.so.1`` /
``liblz4.so.1`` of the image ``dlopen``ed; frames with zstd, lz4, blosclz or zlib inside, byte- or bit-shuffled, are
read -- Zarr's own default ``Blosc(lz4, 5, SHUFFLE)`` included; zstd frames are written, and byte-shuffled LZ4 frames of
2-byte elements by the library's own LZ4 block encoder, ``csrc/dsx_lz4_enc.h``).  Pinned by frames of the
real c-blosc 1.21.0 (``tests/golden/blosc_frames.npz``, ``oracle/make_golden_blosc.py``).
"""

import itertools
import json
import os
import zlib

import numpy as np

CODEC_RAW, CODEC_ZLIB, CODEC_BLOSC = 0, 1, 2  # DSX_CODEC_* of include/dsx.h
# numcodecs.Blosc(cname="zstd", clevel=3, shuffle=Blosc.SHUFFLE).get_config(), zarr_destriper.py:1066-1074
BLOSC_ZSTD = {"id": "blosc", "cname": "zstd", "clevel": 3, "shuffle": 1, "blocksize": 0}
# The digest manifest of an array (csrc/dsx_digest.h, integrity.py): two files in the array's folder that Zarr readers
# ignore.  The JSON names the geometry the records belong to; the binary file holds one record (count, sum, wsum: three
# little-endian uint64) per chunk in C order of the chunk grid, zero-filled at creation: count == 0 is "not recorded".
DIGEST_JSON, DIGEST_BIN = ".dsxdigest.json", ".dsxdigest.bin"
DIGEST_FORMAT, DIGEST_ALGORITHM, DIGEST_RECORD_BYTES = 1, "dsx-sm64-rowcol", 24


def _native():
    from . import engine

    return engine.load_library()


def blosc_decode(frame, nbytes):
    """One Blosc frame -> ``bytes`` object of ``nbytes`` (``dsx_blosc_decode``)."""
    import ctypes

    lib = _native()
    out = ctypes.create_string_buffer(nbytes)
    rc = lib.dsx_blosc_decode(frame, len(frame), out, nbytes)
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"blosc: decode failed").decode())
    return out.raw


def blosc_encode(raw, typesize, clevel=3, shuffle=True, cname="zstd"):
    """Bytes-like -> one Blosc frame with zstd inside (``dsx_blosc_encode``), or, for ``cname="lz4"`` (2-byte elements,
    byte shuffle only), with LZ4 inside and split streams (``dsx_blosc_encode_lz4``)."""
    import ctypes

    if cname not in ("zstd", "lz4"):
        raise NotImplementedError("Blosc frames are written with zstd or lz4 inside; cname {!r} is read-only".format(cname))
    if cname == "lz4" and (int(typesize) != 2 or not shuffle):
        raise NotImplementedError("Blosc-LZ4 frames are written byte-shuffled at typesize 2 only")
    lib = _native()
    raw = bytes(raw)
    out = ctypes.create_string_buffer(len(raw) + 16)
    n = ctypes.c_size_t()
    if cname == "lz4":
        rc = lib.dsx_blosc_encode_lz4(raw, len(raw), int(clevel), out, len(raw) + 16, ctypes.byref(n))
    else:
        rc = lib.dsx_blosc_encode(raw, len(raw), int(typesize), int(clevel), 1 if shuffle else 0, out, len(raw) + 16,
                                  ctypes.byref(n))  # fmt: skip
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"blosc: encode failed").decode())
    return out.raw[: n.value]


def digest_grid_of(shape, chunks, dtype):
    """The chunk grid ``(g0, g1, g2)`` a digest manifest covers: a uint16 array whose last three axes are ``(Z, Y, X)``
    and whose leading axes have length 1 with chunk 1.  Anything else is a ``ValueError``."""
    shape, chunks = tuple(int(x) for x in shape), tuple(int(x) for x in chunks)
    if np.dtype(dtype) != np.uint16:
        raise ValueError("digests cover uint16 arrays, not {}".format(np.dtype(dtype)))
    if len(shape) < 3 or len(chunks) != len(shape) or any(n != 1 or c != 1 for n, c in zip(shape[:-3], chunks[:-3])):
        raise ValueError("digests need (Z, Y, X) as the last three axes and leading axes of length 1 with chunk 1, "
                         "got shape {} chunks {}".format(shape, chunks))  # fmt: skip
    if any(n < 1 or c < 1 for n, c in zip(shape[-3:], chunks[-3:])):
        raise ValueError("digests need a non-empty array, got shape {} chunks {}".format(shape, chunks))
    return tuple(-(-n // c) for n, c in zip(shape[-3:], chunks[-3:]))


class MiniZarrArray:
    def __init__(self, path, meta):
        self.path = str(path)
        self.shape = tuple(meta["shape"])
        self.chunks = tuple(meta["chunks"])
        self.dtype = np.dtype(meta["dtype"])
        self.fill_value = meta.get("fill_value", 0) or 0
        self.sep = meta.get("dimension_separator", ".")
        comp = meta.get("compressor")
        self.compressor_meta = None if comp is None else dict(comp)  # as written in .zarray (matches())
        if comp is None:
            self.compressor = None
        elif comp.get("id") == "zlib":
            self.compressor = ("zlib", int(comp.get("level", 1)))
        elif comp.get("id") == "blosc":
            # reading only needs the frames (their headers name the inner codec); writing: blosc_write_params
            self.compressor = ("blosc", int(comp.get("clevel", 5)), str(comp.get("cname", "lz4")),
                               int(comp.get("shuffle", 1)))  # fmt: skip
            self._blosc_blocksize = int(comp.get("blocksize", 0) or 0)
        else:
            raise NotImplementedError(
                "compressor {!r} is not available (null / zlib / blosc are)".format(comp.get("id"))
            )
        if meta.get("order", "C") != "C" or meta.get("filters"):
            raise NotImplementedError("only C-order arrays without filters are supported")
        self.ndim = len(self.shape)
        self._dirs_made = set()
        self.digest_grid = self._load_manifest()  # (g0, g1, g2) of an array that keeps a digest manifest, else None

    @property
    def codec(self):
        """``DSX_CODEC_*`` of the chunk files (``dsx_io_read_chunks``)."""
        return {None: CODEC_RAW, "zlib": CODEC_ZLIB, "blosc": CODEC_BLOSC}[self.compressor and self.compressor[0]]

    def blosc_write_params(self):
        """``(clevel, typesize, byte shuffle)`` for ``dsx_io_write_chunks_blosc``, or ``(clevel, 2, True, "lz4")`` for
        ``dsx_io_write_chunks_blosc_lz4`` (``Engine.io_write_chunks(blosc=...)``); raises for what the writers lack."""
        _, clevel, cname, shuffle = self.compressor
        if cname == "lz4":
            if self.dtype.itemsize != 2 or shuffle not in (1, -1) or self._blosc_blocksize:
                raise NotImplementedError("Blosc-LZ4 frames are written for 2-byte elements with byte shuffle and "
                                          "blocksize 0 only; this array's compressor is read-only")
            return clevel, 2, True, "lz4"
        if cname != "zstd":
            raise NotImplementedError("Blosc frames are written with zstd or lz4 inside; cname {!r} is read-only".format(cname))
        if shuffle == 2 or (shuffle == -1 and self.dtype.itemsize == 1):
            raise NotImplementedError("Blosc bit-shuffle is not implemented")
        return clevel, self.dtype.itemsize, shuffle != 0

    def _decode(self, raw):
        if self.compressor is None:
            return raw
        if self.compressor[0] == "zlib":
            return zlib.decompress(raw)
        return blosc_decode(raw, int(np.prod(self.chunks)) * self.dtype.itemsize)

    def _encode(self, raw):
        if self.compressor is None:
            return raw
        if self.compressor[0] == "zlib":
            return zlib.compress(raw, self.compressor[1])
        clevel, typesize, shuffle, *cname = self.blosc_write_params()
        return blosc_encode(raw, typesize, clevel, shuffle, *cname)

    # -- construction -------------------------------------------------------------------------
    @staticmethod
    def _compressor_meta(compressor):
        """The ``compressor`` entry of ``.zarray`` for what :meth:`create` accepts."""
        if compressor is None:
            return None
        if compressor == "zlib":
            return {"id": "zlib", "level": 1}
        if compressor == "blosc":
            return dict(BLOSC_ZSTD)
        if isinstance(compressor, dict):
            return dict(compressor)  # a numcodecs get_config() dict
        raise NotImplementedError("compressors: None, 'zlib', 'blosc' or a numcodecs config dict")

    @classmethod
    def create(cls, path, shape, chunks, dtype, compressor=None, dimension_separator="/", fill_value=0,
               overwrite=True, digests=False):  # fmt: skip
        """``digests``: keep a digest manifest next to the chunks (``.dsxdigest.json`` / ``.dsxdigest.bin``): one record
        per chunk, kept truthful by every write through this class and filled by the store pass from the device.  Needs
        a uint16 array whose leading axes (all but the last three) have length 1 and chunk 1, else ``ValueError``.  A
        manifest left by an earlier array at ``path`` is removed whenever the array is (re)created."""
        if digests:
            digest_grid_of(shape, chunks, dtype)  # (refuses what the digest does not cover before anything is touched)
        os.makedirs(path, exist_ok=True)
        if not overwrite and os.path.exists(os.path.join(path, ".zarray")):
            raise FileExistsError(path)
        for name in (DIGEST_JSON, DIGEST_BIN):  # an overwritten store never keeps an old manifest
            try:
                os.remove(os.path.join(path, name))
            except FileNotFoundError:
                pass
        comp = cls._compressor_meta(compressor)
        meta = {
            "zarr_format": 2,
            "shape": list(shape),
            "chunks": list(chunks),
            "dtype": np.dtype(dtype).str,
            "compressor": comp,
            "fill_value": fill_value,
            "order": "C",
            "filters": None,
            "dimension_separator": dimension_separator,
        }
        # written to a temporary name and renamed: a concurrent reader (another rank polling for the array)
        # sees the metadata either whole or not at all
        tmp = os.path.join(path, ".zarray.tmp.{}".format(os.getpid()))
        if digests:  # before .zarray appears: a rank that sees the array sees its manifest
            grid = digest_grid_of(shape, chunks, dtype)
            with open(os.path.join(path, DIGEST_BIN), "wb") as f:
                f.truncate(grid[0] * grid[1] * grid[2] * DIGEST_RECORD_BYTES)
            with open(tmp, "w") as f:
                json.dump({"format": DIGEST_FORMAT, "algorithm": DIGEST_ALGORITHM, "shape": list(shape),
                           "chunks": list(chunks), "dtype": np.dtype(dtype).str, "fill_value": fill_value,
                           "grid": list(grid)}, f)  # fmt: skip
            os.replace(tmp, os.path.join(path, DIGEST_JSON))
        with open(tmp, "w") as f:
            json.dump(meta, f)
        os.replace(tmp, os.path.join(path, ".zarray"))
        return cls(path, meta)

    @classmethod
    def open(cls, path):
        with open(os.path.join(path, ".zarray")) as f:
            return cls(path, json.load(f))

    def matches(self, shape, chunks, dtype, compressor=Ellipsis):
        """Does this array have the given geometry -- and, when ``compressor`` is given (what :meth:`create` takes),
        the given codec?  Tells the array rank 0 has just created from a stale one: a left-over of an earlier run with
        ANOTHER codec has the same geometry, and a rank that opened it would write chunks the new metadata cannot read."""
        ok = (self.shape == tuple(int(x) for x in shape) and self.chunks == tuple(int(x) for x in chunks)
              and self.dtype == np.dtype(dtype))
        if ok and compressor is not Ellipsis:
            ok = self.compressor_meta == self._compressor_meta(compressor)
        return ok

    # -- digest manifest ----------------------------------------------------------------------
    def _load_manifest(self):
        """The chunk grid of this array's manifest, or ``None``: no manifest, or one of another array (which a reader
        must not trust; ``create`` removes it)."""
        try:
            with open(os.path.join(self.path, DIGEST_JSON)) as f:
                man = json.load(f)
        except (FileNotFoundError, ValueError):
            return None
        try:
            grid = digest_grid_of(self.shape, self.chunks, self.dtype)
        except ValueError:
            return None
        same = (man.get("format") == DIGEST_FORMAT and man.get("algorithm") == DIGEST_ALGORITHM
                and tuple(man.get("shape", ())) == self.shape and tuple(man.get("chunks", ())) == self.chunks
                and man.get("dtype") == self.dtype.str and tuple(man.get("grid", ())) == grid
                and (man.get("fill_value", 0) or 0) == self.fill_value)  # fmt: skip
        return grid if same and os.path.exists(os.path.join(self.path, DIGEST_BIN)) else None

    def digest_extents(self, idx3):
        """Valid extents of the chunk at grid position ``idx3`` (last three axes): the part inside the array."""
        return tuple(min(c, n - g * c) for c, n, g in zip(self.chunks[-3:], self.shape[-3:], idx3))

    def digest_records(self):
        """The manifest's records: ``engine.DIGEST_DTYPE[g0 * g1 * g2]`` in C order of the chunk grid (a copy);
        ``count == 0`` marks a chunk nobody recorded.  ``ValueError`` when the array keeps no manifest."""
        from . import engine

        if self.digest_grid is None:
            raise ValueError("{} keeps no digest manifest".format(self.path))
        n = int(np.prod(self.digest_grid))
        rec = np.fromfile(os.path.join(self.path, DIGEST_BIN), dtype=engine.DIGEST_DTYPE)
        if rec.size != n:
            raise ValueError("{}: {} records, the chunk grid has {}".format(os.path.join(self.path, DIGEST_BIN), rec.size, n))
        return rec

    def set_digest_records(self, first_chunk_row, records):
        """Store the records of whole chunk rows (a row: the ``g1 * g2`` chunks of one z position) from chunk row
        ``first_chunk_row`` on: one contiguous byte range of the file, so writers of disjoint rows -- the blocks of a
        pass, the ranks of a job -- never touch each other's bytes and nothing is merged."""
        from . import engine

        if self.digest_grid is None:
            raise ValueError("{} keeps no digest manifest".format(self.path))
        rec = np.ascontiguousarray(records, dtype=engine.DIGEST_DTYPE).reshape(-1)
        row = self.digest_grid[1] * self.digest_grid[2]
        first = int(first_chunk_row)
        if first < 0 or rec.size % row or first + rec.size // row > self.digest_grid[0]:
            raise ValueError("digest records: {} records from chunk row {} do not fit the grid {}".format(
                rec.size, first, self.digest_grid))  # fmt: skip
        self._put_records(first * row, rec)

    def _put_records(self, first_chunk, rec):
        fd = os.open(os.path.join(self.path, DIGEST_BIN), os.O_WRONLY)
        try:
            os.pwrite(fd, rec.tobytes(), first_chunk * DIGEST_RECORD_BYTES)
        finally:
            os.close(fd)

    def _record_chunk(self, idx, block):
        """(an array with a manifest) The record of the chunk ``block`` about to be stored at ``idx``, host build."""
        from . import engine

        idx3 = tuple(int(i) for i in idx[-3:])
        rec = engine.brick_digest_ref(block, (1, 1, 1), self.chunks[-3:], self.digest_extents(idx3))
        g = self.digest_grid
        self._put_records((idx3[0] * g[1] + idx3[1]) * g[2] + idx3[2], rec)

    # -- chunk io -----------------------------------------------------------------------------
    def _chunk_path(self, idx):
        return os.path.join(self.path, self.sep.join(str(i) for i in idx).replace("/", os.sep))

    def _read_chunk(self, idx):
        p = self._chunk_path(idx)
        if not os.path.exists(p):
            return np.full(self.chunks, self.fill_value, dtype=self.dtype)
        with open(p, "rb") as f:
            raw = self._decode(f.read())
        return np.frombuffer(raw, dtype=self.dtype).reshape(self.chunks).copy()

    def read_chunk_into(self, idx, out_flat):
        """Decompressed chunk ``idx`` (the whole brick, as stored) into a flat array of chunk size."""
        p = self._chunk_path(idx)
        try:
            f = open(p, "rb", buffering=0)
        except FileNotFoundError:
            out_flat[...] = self.fill_value
            return
        with f:
            if self.compressor is None:
                # raw chunk: straight into the (pinned) staging buffer, one copy, no GIL held by the read
                view = memoryview(out_flat).cast("B")
                got = f.readinto(view)
                if got != len(view):
                    raise ValueError("chunk {} has {} bytes, expected {}".format(p, got, len(view)))
                return
            raw = self._decode(f.read())
        out_flat[...] = np.frombuffer(raw, dtype=self.dtype)

    def write_chunk_flat(self, idx, flat):
        """Store a whole brick given in chunk (C) order."""
        self._write_chunk(idx, np.asarray(flat, dtype=self.dtype))

    def _write_chunk(self, idx, block):
        p = self._chunk_path(idx)
        d = os.path.dirname(p)
        if d not in self._dirs_made:
            os.makedirs(d, exist_ok=True)
            self._dirs_made.add(d)
        block = np.ascontiguousarray(block, dtype=self.dtype)
        raw = self._encode(memoryview(block).cast("B"))
        with open(p + ".tmp", "wb", buffering=0) as f:
            f.write(raw)
        os.replace(p + ".tmp", p)
        if self.digest_grid is not None:  # the manifest stays truthful whoever writes the chunk
            self._record_chunk(idx, block)

    # -- slicing ------------------------------------------------------------------------------
    def _normalize(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        if any(k is Ellipsis for k in key):
            i = key.index(Ellipsis)
            key = key[:i] + (slice(None),) * (self.ndim - len(key) + 1) + key[i + 1 :]
        key = key + (slice(None),) * (self.ndim - len(key))
        out, squeeze = [], []
        for ax, (k, n) in enumerate(zip(key, self.shape)):
            if isinstance(k, (int, np.integer)):
                k = int(k) + (n if k < 0 else 0)
                out.append((k, k + 1))
                squeeze.append(ax)
            else:
                start, stop, step = k.indices(n)
                if step != 1:
                    raise NotImplementedError("only unit steps")
                out.append((start, max(start, stop)))
        return out, tuple(squeeze)

    def _chunk_ranges(self, bounds):
        return [range(lo // c, (hi - 1) // c + 1) if hi > lo else range(0) for (lo, hi), c in zip(bounds, self.chunks)]

    def __getitem__(self, key):
        bounds, squeeze = self._normalize(key)
        out = np.empty([hi - lo for lo, hi in bounds], dtype=self.dtype)
        for idx in itertools.product(*self._chunk_ranges(bounds)):
            chunk = self._read_chunk(idx)
            src, dst = [], []
            for (lo, hi), c, i in zip(bounds, self.chunks, idx):
                a, b = max(lo, i * c), min(hi, (i + 1) * c)
                src.append(slice(a - i * c, b - i * c))
                dst.append(slice(a - lo, b - lo))
            out[tuple(dst)] = chunk[tuple(src)]
        return out.squeeze(axis=squeeze) if squeeze else out

    def __setitem__(self, key, value):
        bounds, _ = self._normalize(key)
        shape = [hi - lo for lo, hi in bounds]
        # NumPy assignment cast, as zarr does: float -> uint16 truncates (zarr_destriper.py:336)
        value = np.broadcast_to(np.asarray(value), shape) if np.ndim(value) else np.full(shape, value)
        value = value.astype(self.dtype, copy=False)
        for idx in itertools.product(*self._chunk_ranges(bounds)):
            src, dst, full = [], [], True
            for (lo, hi), c, i, n in zip(bounds, self.chunks, idx, self.shape):
                a, b = max(lo, i * c), min(hi, (i + 1) * c)
                dst.append(slice(a - i * c, b - i * c))
                src.append(slice(a - lo, b - lo))
                full = full and (a == i * c) and (b == min((i + 1) * c, n))
            if full and all(s.stop - s.start == c for s, c in zip(dst, self.chunks)):
                chunk = value[tuple(src)]
            else:
                chunk = self._read_chunk(idx)
                chunk[tuple(dst)] = value[tuple(src)]
            self._write_chunk(idx, chunk)
