"""Zarr chunk map of the reference with the per-plane z-loop replaced by one batched GPU call.

Mirrors the boundary of ``/root/reference/code/aind_smartspim_destripe/zarr_destriper.py`` that the
hot path sees: :func:`execute_worker` (reference ``:253-336``) has the reference's signature and
writes the filtered block into the output array exactly where the reference does.  The producer /
consumer process pool (``:797-906``) becomes a plain loop over z-blocks per rank
(:func:`destripe_zarr_store`): one process per GPU owns a contiguous, chunk-aligned z-range
(``distributed.z_shard``), so no queue and no pickled 819 MB blocks are needed.

The two public entry points above it keep the reference's parameter lists -- :func:`destripe_channel`
(``:1214-1223``, called by keyword from ``run_capsule.py:394-403``) and :func:`destripe_zarr` (``:909-924``) -- with
the engine's extras keyword-only behind them, and ``compute_pyramid`` / ``compute_multiscale`` are reachable under
the reference's module name (``tests/test_reference_signatures.py`` holds every same-named function to the
reference's signature).

``recover_global_position`` / ``unpad_global_coords`` belong to the third-party package
``aind_large_scale_prediction==1.0.0`` (``zarr_destriper.py:22-24``), which is not vendored in the
reference and not installed here; their behaviour is restated from the call site (``:268-312``) and is
exact for the production setting ``overlap_prediction_chunksize=(0, 0, 0)`` (``:1018-1022``).

Row f1 of SURVEY section 8: when the store holds uint16 bricks, :func:`destripe_zarr_store` uploads the
decompressed chunks as they lie in the store and re-tiles them into planes (and the filtered planes back
into bricks) on the device (``dsx_bricks_to_planes_u16`` / ``dsx_planes_to_bricks_u16``), so the host only
(de)compresses -- no NumPy gather / scatter of 128 x 128 tiles.  The multiscale pyramid is in ``pyramid.py``.
The OME-NGFF metadata of the group (``:410-674``) is written on request (``ome_metadata=True``), with the display window
the reference hard-codes or the percentiles of an exact device histogram of the written voxels.
Out of scope here: the psutil profiler.
"""

import itertools
import json
import logging
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from pathlib import Path

import numpy as np

from . import engine as engine_mod
from . import filtering as fl
from .distributed import z_shard
from . import mini_tiff as tif
from .mini_zarr import MiniZarrArray


# ---------------------------------------------------------------------------------------------
# Shading plumbing around the filter
# ---------------------------------------------------------------------------------------------
def read_json_as_dict(filepath: str) -> dict:
    """``utils/utils.py:414-446``: ``{}`` for a missing file; a second, lossy decode on ``UnicodeDecodeError``."""
    dictionary = {}
    if os.path.exists(filepath):
        try:
            with open(filepath) as json_file:
                dictionary = json.load(json_file)
        except UnicodeDecodeError:
            print("Error reading json with utf-8, trying different approach")
            with open(filepath, "rb") as json_file:
                data = json_file.read()
                dictionary = json.loads(data.decode("utf-8", errors="ignore"))
    return dictionary


def _natsorted(names):
    """Natural order of file names (``natsort.natsorted`` default: digit runs compare as integers)."""
    key = lambda s: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", str(s))]  # noqa: E731
    return sorted(names, key=key)


def _emission_wavelength(channel_name):
    """First all-digit token of ``Ex_561_Em_593``-style channel names, or ``None``."""
    for token in str(channel_name).split("_"):
        if token.isdigit():
            return int(token)
    return None


def _tile_sides(tile_config, wavelength):
    """``{X folder: {Y folder: brain side}}`` of the tiles imaged with ``wavelength``."""
    sides = {}
    for entry in tile_config.values():
        if int(entry.get("Laser")) != wavelength:
            continue
        try:
            x_folder, y_folder, side = (entry[k] for k in ("X", "Y", "Side"))
            if x_folder is None or y_folder is None or side is None:
                raise KeyError
        except KeyError:
            raise KeyError("Please, check the data in metadata.json") from None
        sides.setdefault(x_folder, {})[y_folder] = int(side)
    return sides


def get_microscope_flats(channel_name: str, derivatives_folder):
    """Microscope flats of a channel (reference ``zarr_destriper.py:70-154``).

    Returns ``([flat of side 0, flat of side 1], {X folder: {Y folder: side}})`` read from
    ``<derivatives>/FlatReal<wavelength>_*.tif`` (natural file order) and ``metadata.json``'s ``tile_config``;
    ``(None, None)`` when there is no ``metadata.json`` or the channel name holds no wavelength.
    ``ValueError`` without ``tile_config`` or unless exactly two flats exist; ``KeyError`` for a tile entry
    without ``X`` / ``Y`` / ``Side``.
    """
    folder = Path(derivatives_folder)
    wavelength = _emission_wavelength(channel_name)
    meta_path = folder / "metadata.json"
    if wavelength is None or not meta_path.exists():
        return None, None
    tile_config = read_json_as_dict(filepath=meta_path).get("tile_config")
    if tile_config is None:
        raise ValueError("Please, verify metadata.json")
    sides = _tile_sides(tile_config, wavelength)
    flat_files = _natsorted(glob(f"{folder}/FlatReal{wavelength}_*.tif"))
    flats = [tif.imread(f) for f in flat_files if os.path.exists(f)]
    if len(flats) != 2:
        raise ValueError(f"Error while reading the microscope flatfields: {flats}")
    return flats, sides


def load_shadow_correction(derivatives_path, output_destriped_zarr, flatfield=None, logger=None):
    """The ``shadow_correction`` dict ``destripe_zarr`` hands to the filter (reference ``zarr_destriper.py:1095-1130``).

    ``darkfield`` = ``<derivatives>/DarkMaster_cropped.tif`` (``FileNotFoundError`` with the reference's message if
    the folder exists but the file does not; ``None`` if there is no derivatives folder at all).  A given
    ``flatfield`` is the retrospective one; otherwise the microscope flats of the channel (the folder above
    the tile) are loaded, normalised, and returned with their tile config.
    """
    log = logger or logging.getLogger("dsx.zarr")
    folder = Path(derivatives_path)
    correction = {"retrospective": flatfield is not None, "flatfield": flatfield, "darkfield": None, "tile_config": None}
    if not os.path.exists(folder):
        return correction
    dark_file = str(folder / "DarkMaster_cropped.tif")
    log.info(f"Loading darkfield from path: {dark_file}")
    if not os.path.exists(dark_file):
        raise FileNotFoundError(f"Please, provide the current dark from the microscope! Provided path: {dark_file}")
    correction["darkfield"] = tif.imread(dark_file)
    if flatfield is not None:
        log.info("Ignoring microscope flats...")
        return correction
    channel = Path(output_destriped_zarr).parent.name
    flats, correction["tile_config"] = get_microscope_flats(channel_name=str(channel), derivatives_folder=folder)
    correction["flatfield"] = fl.normalize_image(flats)
    return correction


def pad_array_n_d(arr, dim: int = 5):
    """Leading singleton axes up to ``dim`` dimensions (reference ``zarr_destriper.py:157-179``; at most 5)."""
    if dim > 5:
        raise ValueError("Padding more than 5 dimensions is not supported.")
    missing = max(0, dim - arr.ndim)
    return arr.reshape((1,) * missing + arr.shape)


def recover_global_position(super_chunk_slice, internal_slices):
    """Global (z, y, x) slices of a block = super-chunk origin + position inside the super chunk.

    Restated from the call site ``zarr_destriper.py:268-275`` (third-party helper).
    Returns ``(global_slices, starts, stops)``.
    """
    internal = internal_slices[0] if isinstance(internal_slices, (list,)) else internal_slices
    glob = tuple(
        slice(int(sc.start) + int(it.start), int(sc.start) + int(it.stop))
        for sc, it in zip(tuple(super_chunk_slice)[-3:], tuple(internal)[-3:])
    )
    return glob, tuple(s.start for s in glob), tuple(s.stop for s in glob)


def unpad_global_coords(global_coord_pos, block_shape, overlap_prediction_chunksize, dataset_shape):
    """Drop the overlap halo of a block except at the dataset border (call site ``:277-282``).

    Returns ``(unpadded_global_slices, unpadded_local_slices)`` (3 slices each).
    """
    dshape = tuple(dataset_shape)[-3:]
    glob_out, loc_out = [], []
    for g, n, ov, d in zip(tuple(global_coord_pos)[-3:], tuple(block_shape)[-3:], overlap_prediction_chunksize, dshape):
        lo = int(ov) if g.start > 0 else 0
        hi = int(ov) if g.stop < d else 0
        glob_out.append(slice(g.start + lo, g.stop - hi))
        loc_out.append(slice(lo, n - hi))
    return tuple(glob_out), tuple(loc_out)


def execute_worker(
    data,
    batch_super_chunk,
    batch_internal_slice,
    cells_config,
    no_cells_config,
    overlap_prediction_chunksize,
    output_destriped_zarr,
    shadow_correction,
    dataset_name,
    logger: logging.Logger,
    device: int = 0,
    max_batch: int = 64,
    streaks=None,
    *,
    rotate: bool = False,
    lightsheet=None,
):
    """``zarr_destriper.py:253-336`` with the plane loop (``:319-327``) as one batched GPU call.

    ``lightsheet`` (the checked dict of ``fl.lightsheet_options``): the uint16 planes go through the light-sheet
    background mode (``fl.correct_lightsheet_planes``) instead; configs and ``shadow_correction`` are not read then.

    ``rotate``: every plane is filtered as ``np.rot90(F(np.rot90(x)), -1)`` (vertical stripes; the turns run on the
    device, ``fl.destripe_planes``); a ``"rotate"`` key of ``streaks`` asks for the same.

    ``streaks`` (the checked dict of ``fl.streaks_options``, ``route`` resolved): the planes go through the dual-band
    filter (``fl.destripe_streaks_planes``) instead; the configs are not read then, and the ``shadow_correction`` is
    resolved as for the stripe filter and applied when the dict says ``"shading": True``.

    ``data``: float32 (or uint16) ``[1, Z, Y, X]``; every plane goes through ``filter_stripes`` semantics
    with ``microscope_high_int=2500`` (``:326``); the result is assigned to
    ``output_destriped_zarr[output_slices]`` (uint16 store: truncation, ``:336``).
    """
    rotate = engine_mod.rotate_flag(rotate)
    data = np.squeeze(data, axis=0)
    global_coord_pos, _, _ = recover_global_position(batch_super_chunk, batch_internal_slice)
    unpadded_global_slice, unpadded_local_slice = unpad_global_coords(
        global_coord_pos=global_coord_pos,
        block_shape=data.shape,
        overlap_prediction_chunksize=overlap_prediction_chunksize,
        dataset_shape=output_destriped_zarr.shape,
    )
    lead = (slice(0, 1),) * (len(output_destriped_zarr.shape) - 3)
    unpadded_local_slice = list(lead + tuple(unpadded_local_slice))
    output_slices = list(lead + tuple(unpadded_global_slice))
    for idx in range(len(output_destriped_zarr.shape)):  # clip at the dataset border (:301-309)
        if output_slices[idx].stop > output_destriped_zarr.shape[idx]:
            rest = output_slices[idx].stop - output_destriped_zarr.shape[idx]
            unpadded_local_slice[idx] = slice(unpadded_local_slice[idx].start, unpadded_local_slice[idx].stop - rest)
            output_slices[idx] = slice(output_slices[idx].start, output_destriped_zarr.shape[idx])

    input_tile_path = dataset_name.replace(".zarr", "")
    planes = data if data.dtype in (np.uint16, np.float32) else data.astype(np.float32)
    if lightsheet is not None:
        filtered = fl.correct_lightsheet_planes(data, rotate=rotate, out_dtype=np.uint16, max_batch=max_batch,
                                                device=device, **lightsheet)  # fmt: skip
    elif streaks is not None:
        flat, dark = fl._resolve_shading(shadow_correction, input_tile_path)
        kw = fl.streaks_call_options(streaks, flat, dark)
        kw["rotate"] = rotate or engine_mod.rotate_flag(kw.get("rotate", False))
        filtered = fl.destripe_streaks_planes(planes, out_dtype=np.uint16, max_batch=max_batch, device=device, **kw)
    else:
        filtered = fl.destripe_planes(
            planes,
            input_tile_path=input_tile_path,
            no_cells_config=no_cells_config,
            cells_config=cells_config,
            shadow_correction=shadow_correction,
            microscope_high_int=2500,
            out_dtype=np.uint16,
            max_batch=max_batch,
            device=device,
            rotate=rotate,
        )
    if filtered.shape != data.shape:
        # odd planes grow by one row / column (waverec2); the reference's assignment into
        # np.zeros_like(data) would raise here -- keep the part that maps onto the input grid
        filtered = filtered[:, : data.shape[1], : data.shape[2]]
    block = pad_array_n_d(filtered[tuple(unpadded_local_slice[-3:])], dim=len(output_destriped_zarr.shape))
    output_destriped_zarr[tuple(output_slices)] = block
    return block  # (the reference returns nothing; the chunk map counts what was assigned: ``histogram``)


def iter_blocks(zyx_shape, prediction_chunksize, z_range=None):
    """Producer analogue (``:797-843``): blocks in z-major order as (super_chunk, internal_slice)."""
    Z, Y, X = zyx_shape
    cz, cy, cx = prediction_chunksize
    z0, z1 = (0, Z) if z_range is None else z_range
    for z in range(z0, z1, cz):
        for y in range(0, Y, cy):
            for x in range(0, X, cx):
                sc = (slice(z, min(z + cz, z1)), slice(y, min(y + cy, Y)), slice(x, min(x + cx, X)))
                internal = tuple(slice(0, s.stop - s.start) for s in sc)
                yield sc, [internal]


class _DeviceBlocks:
    """Brick-order staging + device re-tiling for one rank (row f1), software-pipelined.

    The reference keeps ``CO_CPUS`` consumer processes busy behind a bounded queue while the producer
    reads ahead (``zarr_destriper.py:797-906, 1138-1172``).  Here the same overlap is three HIP streams
    and two sets of buffers: while block ``b`` is being filtered on the compute stream, the chunks of
    block ``b + 1`` are read / decompressed by the I/O threads and uploaded on the upload stream, and the
    bricks of block ``b - 1`` are downloaded on the download stream and compressed / written by the I/O
    threads.  Host staging is page-locked (``dsx_malloc_host``), so the copies are asynchronous.

    Ordering (``dsx_stream_wait`` = event record + stream wait, nothing blocks the host):
    upload(b) -> compute(b) -> download(b);  upload(b + 2) after compute(b) (it refills the same device
    buffer);  compute(b + 2) after download(b) (it overwrites the same output bricks).  The host waits on
    event slots before it refills a pinned input buffer or hands a pinned output buffer to the writers.

    With ``device_codec`` the output bricks are Blosc-zstd frames before they leave the device
    (``dsx_blosc_encode_device`` on the compute stream, after ``planes_to_bricks``): the download stream brings back
    the frame offsets, then only the packed frames, and the I/O threads write each byte range as it is.

    With ``device_decode`` the input chunks are decoded on the device: the I/O threads only read the files and pack
    the Blosc frames back to back with one task per Blosc block (``dsx_io_read_frames``; frames the device does not
    take are decoded there and shipped as copies), the upload stream brings the packed frames and the task table, and
    ``dsx_blosc_decode_device`` fills the input bricks on the compute stream before ``bricks_to_planes``.  Its
    per-task statuses come back on the compute stream and are checked before the block's output reaches the writers.

    With ``pyr`` (``fused_pyramid``) the pyramid levels are built in the same pass: next to ``planes_to_bricks``,
    ``dsx_pyramid_block_u16`` reduces the block's planes (``d_out``) into one chunk row per level, in brick order, at the
    block's z offset inside that row (``pyramid.fused_schedule``).  A row that the block completes leaves the way level 0
    does, in the block's own slot: its encode is enqueued on the compute stream behind the kernel and its download on
    the download stream BEFORE the slot's event is recorded, so the one event covers level 0 and the rows.  The same
    two rules hold for them.  The host hands a pinned row (or its frames) to the writers only after that event, inside
    the ``_write`` of the block, and ``writes[b - 2]`` has returned before block b may flush into the same pinned row
    again (a level flushes at most once per block, and its rows alternate between two buffers).  The kernel refills a
    device row only behind ``stream_wait(compute, download)`` at the top of ``_submit_out``, issued after the host has
    enqueued the encode / download (and, with ``device_codec``, the frame fetch) of the row that used the buffer two
    flushes ago.
    """

    N_BUF = 2

    def __init__(self, eng, src, dst, zyx, block_z, io_threads, device_codec=False, device_decode=False, pyr=None,
                 pyr_scale=(2, 2, 2)):  # fmt: skip
        self.pyr_scale = tuple(pyr_scale)
        self.eng, self.src, self.dst, self.zyx, self.block_z = eng, src, dst, zyx, block_z
        self.pyr_levels, self.pyr_arrays = pyr if pyr else ([], [])
        self.ci, self.co = tuple(src.chunks[-3:]), tuple(dst.chunks[-3:])
        _, H, W = zyx
        grid = lambda c, zspan: (-(-zspan // c[0]), -(-H // c[1]), -(-W // c[2]))  # noqa: E731
        self.gi = grid(self.ci, block_z + self.ci[0] - 1)  # a block may start inside an input chunk
        self.go = grid(self.co, block_z)
        self.in_brick = int(np.prod(self.ci))
        self.out_brick = int(np.prod(self.co))
        in_bytes = int(np.prod(self.gi)) * self.in_brick * 2
        out_bytes = int(np.prod(self.go)) * self.out_brick * 2
        self.decode_mode = device_decode_mode(device_decode)  # None, "zstd", "any" or "full"
        self.device_decode = self.decode_mode is not None
        self.h_in, self.stage_in = [], []
        self.h_packed, self.h_tasks, self.h_status, self.d_packed, self.d_tasks, self.d_status = [], [], [], [], [], []
        if self.device_decode:  # packed frames + task table replace the decompressed staging
            n_in = int(np.prod(self.gi))
            cap = n_in * (self.in_brick * 2 + 16)
            n_tasks = n_in * engine_mod.frame_tasks_per_chunk(self.in_brick * 2)
            self.h_packed = [eng.alloc_host(cap) for _ in range(self.N_BUF)]
            self.h_tasks = [eng.alloc_host(n_tasks * engine_mod.TASK_DTYPE.itemsize) for _ in range(self.N_BUF)]
            self.h_status = [eng.alloc_host(4 * n_tasks) for _ in range(self.N_BUF)]
            self.d_packed = [eng.alloc(cap) for _ in range(self.N_BUF)]
            self.d_tasks = [eng.alloc(n_tasks * engine_mod.TASK_DTYPE.itemsize) for _ in range(self.N_BUF)]
            self.d_status = [eng.alloc(4 * n_tasks) for _ in range(self.N_BUF)]
            self.packed = [h.array((cap,), np.uint8) for h in self.h_packed]
            self.tasks = [h.array((n_tasks,), engine_mod.TASK_DTYPE) for h in self.h_tasks]
            self.status = [h.array((n_tasks,), np.int32) for h in self.h_status]
            self.routes = np.zeros(n_in, np.uint8)  # (one read at a time)
            self.read_info = [None] * self.N_BUF  # (packed bytes, tasks, chunk paths) of the block read into buffer k
            # (tasks, chunk of each task, chunk paths) of the block SUBMITTED from buffer k: the read of block b + 2
            # refills the task table and read_info of buffer k before block b's statuses are checked
            self.decode_info = [None] * self.N_BUF
        else:
            self.h_in = [eng.alloc_host(in_bytes) for _ in range(self.N_BUF)]
            self.stage_in = [h.array(self.gi + (self.in_brick,), np.uint16) for h in self.h_in]
        self.h_out = [eng.alloc_host(out_bytes) for _ in range(self.N_BUF)]
        self.stage_out = [h.array(self.go + (self.out_brick,), np.uint16) for h in self.h_out]
        self.d_bricks_in = [eng.alloc(in_bytes) for _ in range(self.N_BUF)]
        self.d_bricks_out = [eng.alloc(out_bytes) for _ in range(self.N_BUF)]
        self.d_planes = eng.alloc(block_z * H * W * 2)
        self.d_out = eng.alloc(block_z * H * W * 2)
        self.codec_mode = output_codec_mode(device_codec, dst)  # None, "literals", "runs" or "lz4"
        self.device_codec = self.codec_mode is not None
        self.d_frames, self.d_offsets, self.h_frames, self.h_offsets = [], [], [], []
        if self.device_codec:
            n_chunks = int(np.prod(self.go))
            cap = n_chunks * (self.out_brick * 2 + 16)
            self.d_frames = [eng.alloc(cap) for _ in range(self.N_BUF)]
            self.d_offsets = [eng.alloc(8 * (n_chunks + 1)) for _ in range(self.N_BUF)]
            self.h_frames = [eng.alloc_host(cap) for _ in range(self.N_BUF)]
            self.h_offsets = [eng.alloc_host(8 * (n_chunks + 1)) for _ in range(self.N_BUF)]
            self.frames = [h.array((cap,), np.uint8) for h in self.h_frames]
            self.offsets = [h.array((n_chunks + 1,), np.int64) for h in self.h_offsets]
        # fused pyramid: per level two device chunk rows in brick order + what carries a finished row to the host
        self.d_row, self.h_row, self.stage_row, self.pyr_bufs = [], [], [], []
        self.d_pframes, self.d_poffsets, self.h_pframes, self.h_poffsets, self.pframes, self.poffsets = [], [], [], [], [], []
        for lv in self.pyr_levels:
            ny, nx = -(-lv.shape[1] // lv.chunks[1]), -(-lv.shape[2] // lv.chunks[2])
            brick = int(np.prod(lv.chunks))
            row_bytes = ny * nx * brick * 2
            self.d_row.append([eng.alloc(row_bytes) for _ in range(self.N_BUF)])
            if self.device_codec:
                cap = ny * nx * (brick * 2 + 16)
                self.d_pframes.append([eng.alloc(cap) for _ in range(self.N_BUF)])
                self.d_poffsets.append([eng.alloc(8 * (ny * nx + 1)) for _ in range(self.N_BUF)])
                self.h_pframes.append([eng.alloc_host(cap) for _ in range(self.N_BUF)])
                self.h_poffsets.append([eng.alloc_host(8 * (ny * nx + 1)) for _ in range(self.N_BUF)])
                self.pframes.append([h.array((cap,), np.uint8) for h in self.h_pframes[-1]])
                self.poffsets.append([h.array((ny * nx + 1,), np.int64) for h in self.h_poffsets[-1]])
            else:
                self.h_row.append([eng.alloc_host(row_bytes) for _ in range(self.N_BUF)])
                self.stage_row.append([h.array((ny, nx, brick), np.uint16) for h in self.h_row[-1]])
        work = engine_mod.pyramid_work_bytes((block_z, H, W), len(self.pyr_levels) + 1, self.pyr_scale) if self.pyr_levels else 0
        self.d_work = eng.alloc(work) if work else None
        if self.pyr_levels:
            self.pyr_bufs = [b for per_level in (self.d_row + self.h_row + self.d_pframes + self.d_poffsets + self.h_pframes
                                                 + self.h_poffsets) for b in per_level] + ([self.d_work] if work else [])  # fmt: skip
        self.pyr_schedule, self.pyr_cur, self.pyr_flushes = {}, [0] * len(self.pyr_levels), [[] for _ in range(self.N_BUF)]
        self.io_threads = int(io_threads)
        self.timing = _new_timing()
        self.histogram = False  # destripe_zarr_store(histogram=...): count every block's filtered planes (volhist_add)
        # destripe_zarr_store(projections=...): {"output" / "input": device arrays of the rank's z range}, its first
        # plane and the work buffer of one block (eng.project); owned by the call, not by the cached buffers
        self.proj, self.proj_z0, self.proj_work = None, 0, None
        # destripe_zarr_store(digests=True): one record per output chunk of a block and per chunk of a pyramid row, taken
        # on the device behind the re-tiling / pyramid kernel (brick_digest) and carried to the block's writer with the
        # frame offsets (or the bricks).  Allocated by the first call that asks (enable_digests), kept with the buffers.
        self.digests = False
        self.dig_bufs, self.d_dig, self.dig, self.d_pdig, self.pdig = [], [], [], [], []

    def enable_digests(self, on):
        self.digests = bool(on)
        if not on or self.dig_bufs:
            return
        eng, rec, R = self.eng, engine_mod.DIGEST_DTYPE, range(self.N_BUF)

        def pair(n):
            d, h = [eng.alloc(n * rec.itemsize) for _ in R], [eng.alloc_host(n * rec.itemsize) for _ in R]
            self.dig_bufs += d + h
            return d, [b.array((n,), rec) for b in h]

        self.d_dig, self.dig = pair(int(np.prod(self.go)))
        for lv in self.pyr_levels:
            d, h = pair(-(-lv.shape[1] // lv.chunks[1]) * -(-lv.shape[2] // lv.chunks[2]))
            self.d_pdig.append(d)
            self.pdig.append(h)

    def close(self):
        for b in (self.dig_bufs + self.pyr_bufs + self.d_bricks_in + self.d_bricks_out + [self.d_planes, self.d_out] + self.h_in + self.h_out
                  + self.d_frames + self.d_offsets + self.h_frames + self.h_offsets + self.h_packed + self.h_tasks
                  + self.h_status + self.d_packed + self.d_tasks + self.d_status):
            b.free()

    # -- host stages (I/O threads) -------------------------------------------------------------
    def _read(self, z0, z1, k):
        """Decompress the input chunks of planes ``[z0, z1)`` into pinned buffer ``k``."""
        t0 = time.perf_counter()
        lead = (0,) * (self.src.ndim - 3)
        bz0, zoff = divmod(z0, self.ci[0])
        nbz = -(-(zoff + (z1 - z0)) // self.ci[0])
        idx = list(itertools.product(range(nbz), range(self.gi[1]), range(self.gi[2])))
        if self.device_decode:
            paths = [self.src._chunk_path(lead + (bz0 + i[0], i[1], i[2])) for i in idx]
            pb, nt = self.eng.io_read_frames(paths, self.in_brick * 2, self.packed[k], self.tasks[k],
                                             threads=self.io_threads, fill_value=int(self.src.fill_value),
                                             routes=self.routes, mode=ZDEC_MODES[self.decode_mode],
                                             zlib_chunks=self.src.compressor[0] == "zlib")  # fmt: skip
            self.read_info[k] = (pb, nt, paths)
            seen = np.bincount(self.routes[: len(paths)], minlength=3)
            for name, r in (("device", engine_mod.ROUTE_DEVICE), ("host", engine_mod.ROUTE_HOST), ("fill", engine_mod.ROUTE_FILL)):
                self.timing["decode_routes"][name] += int(seen[r])
            self.timing["read_s"] += time.perf_counter() - t0
            return nbz, zoff
        stage = self.stage_in[k]
        paths = [self.src._chunk_path(lead + (bz0 + i[0], i[1], i[2])) for i in idx]
        self.eng.io_read_chunks(paths, [stage[i] for i in idx], threads=self.io_threads,
                                codec=self.src.codec, fill_value=int(self.src.fill_value))  # fmt: skip
        there = sum(os.path.exists(p) for p in paths)  # (what the reader decoded, what it filled)
        self.timing["decode_routes"]["host"] += there
        self.timing["decode_routes"]["fill"] += len(paths) - there
        self.timing["read_s"] += time.perf_counter() - t0
        return nbz, zoff

    def _write_rows(self, flushes):
        """The pyramid chunk rows that left with a block: ``(level index, buffer, chunk row)`` each."""
        for i, j, row in flushes:
            arr, lv = self.pyr_arrays[i], self.pyr_levels[i]
            lead = (0,) * (arr.ndim - 3)
            ny, nx = -(-lv.shape[1] // lv.chunks[1]), -(-lv.shape[2] // lv.chunks[2])
            idx = list(itertools.product(range(ny), range(nx)))
            paths = [arr._chunk_path(lead + (row, y, x)) for y, x in idx]
            if self.device_codec:
                frames, offs = self.pframes[i][j], self.poffsets[i][j]
                self.eng.io_write_chunks(paths, [frames[offs[c] : offs[c + 1]] for c in range(len(idx))],
                                         threads=self.io_threads, zlib_level=-1)  # fmt: skip
            else:
                comp = arr.compressor
                self.eng.io_write_chunks(paths, [self.stage_row[i][j][y, x] for y, x in idx], threads=self.io_threads,
                                         zlib_level=-1 if comp is None else int(comp[1]),
                                         blosc=arr.blosc_write_params() if comp and comp[0] == "blosc" else None)  # fmt: skip
            if self.digests:  # the row's records into its own range of the level's manifest, behind its chunk files
                arr.set_digest_records(row, self.pdig[i][j])

    def _write(self, z0, z1, k, flushes=()):
        """Compress / store the output bricks of planes ``[z0, z1)`` from pinned buffer ``k`` (and the pyramid rows that
        left with the block)."""
        t0 = time.perf_counter()
        try:
            self._write_level0(z0, z1, k)
            if self.digests:  # a z block's chunks are one contiguous range of the manifest
                n = -(-(z1 - z0) // self.co[0]) * self.go[1] * self.go[2]
                self.dst.set_digest_records(z0 // self.co[0], self.dig[k][:n])
            self._write_rows(flushes)
        finally:
            self.timing["write_s"] += time.perf_counter() - t0

    def _write_level0(self, z0, z1, k):
        lead = (0,) * (self.dst.ndim - 3)
        nbo = -(-(z1 - z0) // self.co[0])
        oz0 = z0 // self.co[0]
        out = self.stage_out[k]
        odx = list(itertools.product(range(nbo), range(self.go[1]), range(self.go[2])))
        paths = [self.dst._chunk_path(lead + (oz0 + i[0], i[1], i[2])) for i in odx]
        if self.device_codec:  # finished frames: chunk c is bytes [offsets[c], offsets[c + 1]) of the packed buffer
            frames, offs = self.frames[k], self.offsets[k]
            self.eng.io_write_chunks(paths, [frames[offs[c] : offs[c + 1]] for c in range(len(odx))],
                                     threads=self.io_threads, zlib_level=-1)  # fmt: skip
            return
        comp = self.dst.compressor
        level = -1 if comp is None else int(comp[1])
        self.eng.io_write_chunks([self.dst._chunk_path(lead + (oz0 + i[0], i[1], i[2])) for i in odx],
                                 [out[i] for i in odx], threads=self.io_threads, zlib_level=level,
                                 blosc=self.dst.blosc_write_params() if comp and comp[0] == "blosc" else None)  # fmt: skip

    # -- device stage (asynchronous) -----------------------------------------------------------
    def _submit(self, z0, z1, k, nbz, zoff):
        self._submit_in(z0, z1, k, nbz, zoff)
        self._submit_out(z0, z1, k)

    def _submit_in(self, z0, z1, k, nbz, zoff):
        """Upload(b) and compute(b) up to the filter: nothing here touches the output buffers of block b - 2."""
        from .engine import STREAM_COMPUTE as C, STREAM_UPLOAD as U

        eng, (_, H, W), Z = self.eng, self.zyx, z1 - z0
        if self.device_decode:
            pb, nt, paths = self.read_info[k]
            self.decode_info[k] = (nt, self.tasks[k]["chunk"][:nt].copy(), paths, self.tasks[k]["kind"][:nt].copy())
            if pb:
                eng.copy_h2d_async(self.d_packed[k], self.packed[k][:pb], U)
            if nt:
                eng.copy_h2d_async(self.d_tasks[k], self.tasks[k][:nt], U)
            self.timing["upload_bytes"] += pb + nt * engine_mod.TASK_DTYPE.itemsize
        else:
            eng.copy_h2d_async(self.d_bricks_in[k], self.stage_in[k][:nbz], U)
            self.timing["upload_bytes"] += self.stage_in[k][:nbz].nbytes
        eng.event_record(k, U)            # pinned input buffer k may be refilled once this has passed
        eng.stream_wait(C, U)             # compute(b) after upload(b)
        eng.stream_wait(U, C)             # uploads from now on after compute(b - 1): they refill its buffer
        if self.device_decode:            # the bricks from the frames; the statuses come back in stream order
            eng.blosc_decode_device(self.d_packed[k], pb, self.d_tasks[k], nt, self.d_bricks_in[k], self.d_status[k])
            if nt:
                eng.copy_d2h_async(self.status[k][:nt], self.d_status[k], C)
        eng.bricks_to_planes(self.d_bricks_in[k], self.d_planes, (Z, H, W), self.ci, zoff)
        eng.run_device(self.d_planes, np.uint16, Z, self.d_out, np.uint16, None)
        if self.histogram:                # the block's real planes, where every later stage reads them
            eng.volhist_add(self.d_out, Z * H * W)
        if self.proj is not None:         # one more read of the planes, into rows z0 - proj_z0 .. of the rank's arrays
            for key, d in (("output", self.d_out), ("input", self.d_planes)):
                if key in self.proj:
                    eng.project(d, (Z, H, W), self.proj[key], z_off=z0 - self.proj_z0, first=z0 == self.proj_z0,
                                d_work=self.proj_work)  # fmt: skip

    def _submit_out(self, z0, z1, k):
        """Compute(b) from planes_to_bricks on, and download(b): once pinned output buffer k has been written out."""
        from .engine import STREAM_COMPUTE as C, STREAM_DOWNLOAD as D

        eng, (_, H, W), Z = self.eng, self.zyx, z1 - z0
        eng.stream_wait(C, D)             # (the wait lands before planes_to_bricks:) after download(b - 2 .. b - 1)
        eng.planes_to_bricks(self.d_out, self.d_bricks_out[k], (Z, H, W), self.co, 0)
        nbo = -(-Z // self.co[0])
        if self.digests:                  # the bricks where the encoder / the download reads them
            eng.brick_digest(self.d_bricks_out[k], (nbo, self.go[1], self.go[2]), self.co, (Z, H, W), self.d_dig[k])
        flushes = self.pyr_flushes[k] = self._submit_pyramid(z0, z1)
        if self.device_codec:
            n_chunks = nbo * self.go[1] * self.go[2]
            eng.blosc_encode_device(self.d_bricks_out[k], n_chunks, self.out_brick * 2, self.d_frames[k],
                                    self.d_offsets[k], typesize=2, clevel=int(self.dst.compressor[1]),
                                    mode=self.codec_mode)  # fmt: skip
            eng.stream_wait(D, C)
            eng.copy_d2h_async(self.offsets[k][: n_chunks + 1], self.d_offsets[k], D)
            for i, j, _ in flushes:
                eng.copy_d2h_async(self.poffsets[i][j], self.d_poffsets[i][j], D)
            self._download_digests(k, n_chunks, flushes)
            eng.event_record(self.N_BUF + k, D)  # the frame offsets of block b (and of its rows) are here once this has passed
            return
        eng.stream_wait(D, C)             # download(b) after compute(b)
        eng.copy_d2h_async(self.stage_out[k][:nbo], self.d_bricks_out[k], D)
        self.timing["download_bytes"] += self.stage_out[k][:nbo].nbytes
        for i, j, _ in flushes:
            eng.copy_d2h_async(self.stage_row[i][j], self.d_row[i][j], D)
            self._count_pyramid(self.stage_row[i][j].nbytes)
        self._download_digests(k, nbo * self.go[1] * self.go[2], flushes)
        eng.event_record(self.N_BUF + k, D)  # pinned output buffer k (and the rows) hold block b once this has passed

    def _download_digests(self, k, n_chunks, flushes):
        """(download stream, behind its wait for compute(b)) The records of block b and of the rows it completed."""
        if not self.digests:
            return
        from .engine import STREAM_DOWNLOAD as D

        self.eng.copy_d2h_async(self.dig[k][:n_chunks], self.d_dig[k], D)
        self.timing["download_bytes"] += self.dig[k][:n_chunks].nbytes
        for i, j, _ in flushes:
            self.eng.copy_d2h_async(self.pdig[i][j], self.d_pdig[i][j], D)
            self._count_pyramid(self.pdig[i][j].nbytes)

    def _count_pyramid(self, nbytes):
        self.timing["download_bytes"] += nbytes
        self.timing["pyramid_download_bytes"] += nbytes

    def _submit_pyramid(self, z0, z1):
        """(compute stream, behind the wait that protects the output buffers) The block's share of every pyramid level
        into the levels' current device rows; the rows it completes are encoded (``device_codec``) and returned as
        ``(level index, buffer, chunk row)`` for the download."""
        if not self.pyr_levels:
            return []
        eng, (_, H, W) = self.eng, self.zyx
        shares = self.pyr_schedule[(z0, z1)]
        cur = self.pyr_cur
        eng.pyramid_block(self.d_out, (z1 - z0, H, W), [lv.chunks for lv in self.pyr_levels],
                          [self.d_row[i][cur[i]] for i in range(len(shares))], z0s=[s.offset for s in shares],
                          zero=[s.first for s in shares], rows=[1] * len(shares), d_work=self.d_work,
                          **({} if self.pyr_scale == (2, 2, 2) else {"scale": self.pyr_scale}))  # fmt: skip
        flushes = []
        for i, (s, lv) in enumerate(zip(shares, self.pyr_levels)):
            if not s.flush:
                continue
            j = cur[i]
            if self.digests:  # the finished row with its own valid z extent, before the encoder reads it
                eng.brick_digest(self.d_row[i][j], (1, -(-lv.shape[1] // lv.chunks[1]), -(-lv.shape[2] // lv.chunks[2])),
                                 lv.chunks, (min(lv.chunks[0], lv.shape[0] - s.row * lv.chunks[0]),) + tuple(lv.shape[1:]),
                                 self.d_pdig[i][j])  # fmt: skip
            if self.device_codec:
                n_chunks = -(-lv.shape[1] // lv.chunks[1]) * -(-lv.shape[2] // lv.chunks[2])
                eng.blosc_encode_device(self.d_row[i][j], n_chunks, int(np.prod(lv.chunks)) * 2, self.d_pframes[i][j],
                                        self.d_poffsets[i][j], typesize=2,
                                        clevel=int(self.pyr_arrays[i].compressor[1]), mode=self.codec_mode)  # fmt: skip
            flushes.append((i, j, s.row))
            cur[i] = (j + 1) % self.N_BUF
        return flushes

    def _fetch_frames(self, z0, z1, k):
        """(device codec; the offsets of block [z0, z1) are on the host) Download exactly its packed frames."""
        from .engine import STREAM_DOWNLOAD as D

        n_chunks = -(-(z1 - z0) // self.co[0]) * self.go[1] * self.go[2]
        total = int(self.offsets[k][n_chunks])
        self.timing["download_bytes"] += total + 8 * (n_chunks + 1)
        if total:
            self.eng.copy_d2h_async(self.frames[k][:total], self.d_frames[k], D)
        for i, j, _ in self.pyr_flushes[k]:  # the rows that left with the block: their offsets came with level 0's
            offs = self.poffsets[i][j]
            total = int(offs[-1])
            self._count_pyramid(total + offs.nbytes)
            if total:
                self.eng.copy_d2h_async(self.pframes[i][j][:total], self.d_pframes[i][j], D)
        self.eng.event_record(self.N_BUF + k, D)
        self.eng.event_sync(self.N_BUF + k)

    def _check_decode(self, k):
        """(device decode; block in buffer k has been computed) A malformed frame raises as the host reader would."""
        if not self.device_decode:
            return
        nt, chunk, paths, kinds = self.decode_info[k]
        st = self.status[k][:nt]  # (written on the compute stream: block b + 2 is not submitted yet)
        bad = np.flatnonzero(st)
        if bad.size:
            i = int(bad[0])
            raise ValueError(bad_stream_message(int(kinds[i]), paths[int(chunk[i])], int(st[i]),
                                                self.src.compressor[0] == "zlib"))  # fmt: skip

    def run_range(self, z_start, z_stop):
        """All blocks of ``[z_start, z_stop)`` through the pipeline; returns the number of planes."""
        blocks = [(z, min(z + self.block_z, z_stop)) for z in range(z_start, z_stop, self.block_z)]
        nb = len(blocks)
        if self.pyr_levels:
            from . import pyramid

            self.pyr_schedule = dict(pyramid.fused_schedule(self.pyr_levels, z_start, z_stop, self.block_z, self.pyr_scale))
            self.pyr_cur = [0] * len(self.pyr_levels)
        reader = ThreadPoolExecutor(max_workers=1)   # stage drivers: one read and one write in flight,
        writer = ThreadPoolExecutor(max_workers=1)   # each fanning its chunks out over the I/O pool
        try:
            reads = {b: reader.submit(self._read, *blocks[b], b % self.N_BUF) for b in range(min(self.N_BUF, nb))}
            writes = []
            for b in range(nb):
                k = b % self.N_BUF
                nbz, zoff = reads.pop(b).result()
                if self.device_decode:  # the decode and the filter need not wait for the writers
                    self._submit_in(*blocks[b], k, nbz, zoff)
                if b >= self.N_BUF:
                    writes[b - self.N_BUF].result()  # pinned output buffer k has been written out
                if self.device_decode:
                    self._submit_out(*blocks[b], k)
                else:
                    self._submit(*blocks[b], k, nbz, zoff)
                if b + self.N_BUF < nb:
                    self.eng.event_sync(k)  # upload(b) has left pinned input buffer k
                    reads[b + self.N_BUF] = reader.submit(self._read, *blocks[b + self.N_BUF], k)
                if b >= 1:
                    kp = (b - 1) % self.N_BUF
                    self.eng.event_sync(self.N_BUF + kp)  # download(b - 1) complete
                    self._check_decode(kp)
                    if self.device_codec:
                        self._fetch_frames(*blocks[b - 1], kp)
                    writes.append(writer.submit(self._write, *blocks[b - 1], kp, list(self.pyr_flushes[kp])))
            if nb:
                self.eng.event_sync(self.N_BUF + (nb - 1) % self.N_BUF)
                self._check_decode((nb - 1) % self.N_BUF)
                if self.device_codec:
                    self._fetch_frames(*blocks[nb - 1], (nb - 1) % self.N_BUF)
                writes.append(writer.submit(self._write, *blocks[nb - 1], (nb - 1) % self.N_BUF,
                                            list(self.pyr_flushes[(nb - 1) % self.N_BUF])))
            for w in writes:
                w.result()
        finally:
            reader.shutdown()
            writer.shutdown()
        return sum(z1 - z0 for z0, z1 in blocks)


LAST_RUN = {}  # what the last destripe_zarr_store call of this process resolved to (rank, z-range, codec threads): diagnostics
_BLOCKS = {}  # one set of staging buffers per process: page-locking 2 GB of host memory costs ~0.4 s per call


def _new_timing():
    return {"read_s": 0.0, "write_s": 0.0, "upload_bytes": 0, "download_bytes": 0, "pyramid_download_bytes": 0,
            "decode_routes": {"device": 0, "host": 0, "fill": 0}}  # fmt: skip


def device_codec_mode(device_codec):
    """The encoder mode a ``device_codec`` argument selects: ``None`` (off), ``"literals"`` (any true value that is
    not a string: the entropy-only encoder) or ``"runs"`` (the string ``"runs"``).  Any other string: ``ValueError``."""
    if isinstance(device_codec, str):
        if device_codec != "runs":
            raise ValueError("device_codec is False, True or \"runs\", not {!r}".format(device_codec))
        return "runs"
    return "literals" if device_codec else None


def output_codec_mode(device_codec, output):
    """:func:`device_codec_mode` for one output: an open array, or the ``compressor`` it will be created with (what
    ``MiniZarrArray.create`` takes).  A Blosc-LZ4 output is encoded by the device LZ4 encoder: ``"lz4"`` for a true
    ``device_codec``; ``"runs"`` writes zstd sequences and is a ``ValueError`` there."""
    mode = device_codec_mode(device_codec)
    meta = output.compressor_meta if isinstance(output, MiniZarrArray) else MiniZarrArray._compressor_meta(output)
    if mode is None or not (isinstance(meta, dict) and meta.get("id") == "blosc" and meta.get("cname", "lz4") == "lz4"):
        return mode
    if mode == "runs":
        raise ValueError("device_codec=\"runs\" writes zstd sequences; a Blosc-LZ4 output takes device_codec=True")
    return "lz4"


def device_codec_output_ok(dst):
    """Can ``device_codec`` write the array ``dst``: uint16, Blosc with zstd (byte shuffle) or what the LZ4 writer takes."""
    comp = dst.compressor
    if comp is None or comp[0] != "blosc" or dst.dtype != np.uint16:
        return False
    if comp[2] == "lz4":
        try:
            dst.blosc_write_params()
        except NotImplementedError:
            return False
        return True
    return comp[2] == "zstd" and comp[3] == 1


ZDEC_MODES = {"zstd": engine_mod.ZDEC_ZSTD, "any": engine_mod.ZDEC_ANY, "full": engine_mod.ZDEC_ALL}
_TASK_CODECS = {engine_mod.TASK_LZ4: "lz4", engine_mod.TASK_ZLIB: "zlib", engine_mod.TASK_BLOSCLZ: "blosclz"}


def bad_stream_message(kind, path, status, zlib_chunks=False):
    """The text of the ``ValueError`` for a task of ``kind`` the device decoder gave ``status``: what the host reader
    says of such a chunk (``csrc/dsx_io.h``), and the status."""
    if zlib_chunks:
        return "zlib: bad chunk {} [device decode status {}]".format(path, status)
    return "blosc: bad {} stream ({}) [device decode status {}]".format(_TASK_CODECS.get(kind & 0xFF, "zstd"), path, status)


def device_decode_input_ok(src, decode_mode):
    """Can ``device_decode`` read the store ``src``: a Blosc uint16 store, or with ``"full"`` a plain-zlib one."""
    comp = src.compressor
    return comp is not None and src.dtype == np.uint16 and (comp[0] == "blosc" or (decode_mode == "full" and comp[0] == "zlib"))


def device_decode_mode(device_decode):
    """What a ``device_decode`` argument selects: ``None`` (off), ``"zstd"`` (any true value that is not a string: the
    device takes unsplit zstd streams with byte shuffle or none), ``"full"`` (the string ``"full"``: what ``"any"`` takes
    plus blosclz and zlib inside Blosc, and the chunks of a plain-zlib store) or ``"any"`` (the string ``"any"``: LZ4, split streams
    and bit shuffle too).  Any other string: ``ValueError``."""
    if isinstance(device_decode, str):
        if device_decode not in ("any", "full"):
            raise ValueError("device_decode is False, True or one of \"any\", \"full\", not {!r}".format(device_decode))
        return device_decode
    return "zstd" if device_decode else None


def _device_blocks(eng, src, dst, zyx, block_z, io_threads, device_codec=False, device_decode=False, pyr=None,
                   pyr_scale=(2, 2, 2)):  # fmt: skip
    """Staging buffers for this geometry, reused from the previous tile when nothing but the stores changed
    (a channel is tens of tiles of one shape, ``zarr_destriper.py:1231``)."""
    key = (id(eng), tuple(zyx[1:]), tuple(src.chunks[-3:]), tuple(dst.chunks[-3:]), int(block_z),
           output_codec_mode(device_codec, dst),  # (a zstd and an LZ4 output of one geometry differ here only)
           device_decode_mode(device_decode), tuple((lv.level, lv.shape[1:], lv.chunks) for lv in (pyr[0] if pyr else ())),
           tuple(pyr_scale) if pyr else None)  # fmt: skip
    cached = _BLOCKS.get("blocks")
    if cached is not None and cached[0] == key and cached[1].eng._ctx is not None:
        blocks = cached[1]
        blocks.src, blocks.dst, blocks.zyx, blocks.io_threads = src, dst, zyx, int(io_threads)
        blocks.pyr_levels, blocks.pyr_arrays = pyr if pyr else ([], [])
        blocks.timing = _new_timing()
        return blocks
    if cached is not None:
        try:
            cached[1].close()
        except Exception:  # the engine of the cached buffers may be gone already
            pass
    blocks = _DeviceBlocks(eng, src, dst, zyx, block_z, io_threads, device_codec, device_decode, pyr, pyr_scale)
    _BLOCKS["blocks"] = (key, blocks)
    return blocks


def release_staging():
    """Free the cached staging buffers (pinned host + device memory) of this process."""
    cached = _BLOCKS.pop("blocks", None)
    if cached is not None:
        cached[1].close()


def _device_retile_ok(src, dst, zyx, block_z, z0, z1):
    """The device brick path needs uint16 bricks, even planes and output-chunk-aligned z blocks."""
    co = dst.chunks[-3:]
    return (
        src.dtype == np.uint16
        and all(c == 1 for c in src.chunks[:-3])
        and zyx[1] % 2 == 0
        and zyx[2] % 2 == 0
        and block_z % co[0] == 0
        and z0 % co[0] == 0
        and (z1 % co[0] == 0 or z1 == zyx[0])
    )


def destripe_zarr_store(
    dataset_path,
    output_path,
    cells_config,
    no_cells_config,
    shadow_correction=None,
    prediction_chunksize=(64, 1600, 2000),
    output_chunks=(1, 1, 64, 128, 128),
    rank=0,
    world_size=1,
    device=None,
    compressor="blosc",
    logger=None,
    device_retile=None,
    io_threads=None,
    tile_name=None,
    group=None,
    *,
    device_codec=False,
    device_decode=False,
    pyramid_group=None,
    n_levels=1,
    scale_factor=(2, 2, 2),
    streaks=None,
    histogram=None,
    rotate=False,
    lightsheet=None,
    projections=None,
    digests=False,
):
    """Chunk map of ``destripe_zarr`` (``zarr_destriper.py:909-1211``) over a Zarr-v2 directory store -- the engine-level
    form (explicit configs and ``shadow_correction``); :func:`destripe_zarr` is the entry point with the reference's
    signature and calls this.

    ``compressor``: codec of the output array; the default is the reference's,
    ``Blosc(cname="zstd", clevel=3, shuffle=SHUFFLE)`` (``:1066-1074``); ``None`` (raw chunks), ``"zlib"`` or a
    numcodecs config dict are accepted as well.

    Every rank opens the same input / output arrays and processes its own z-range
    (chunk-aligned, so no two ranks touch one output chunk).  Blocks cover the full Y x X plane in
    production (``prediction_chunksize=(64, 1600, 2000)`` == the tile, ``:1256``); smaller y/x blocks
    would change the result (the filter is per plane), so they are rejected.

    Rank 0 creates the output array -- always anew, as the reference does (``overwrite=True``, ``:1065,1073``);
    the metadata file appears atomically.  ``group`` (anything with ``barrier()``: a
    ``distributed.RankGroup`` / ``FileRendezvous``-based barrier, or a ``torch.distributed`` wrapper)
    orders that creation before the other ranks open the array; without a group they poll until the
    metadata on disk has the geometry AND the codec of THIS run (a stale array of another shape or another
    compressor is never used -- chunks written under stale metadata would not be readable under the new one; a
    left-over with the same geometry and codec is indistinguishable and harmless: rank 0 rewrites the same
    metadata, every rank rewrites its own chunks).  ``device=None`` takes the local rank (``LOCAL_RANK``), not the global one.

    ``io_threads``: native threads that read / decompress and compress / write chunks (default:
    :func:`default_io_threads` -- the cores this process may run on divided among the ranks of the node).

    ``device_retile``: ``True`` = chunks are re-tiled into planes and back on the GPU (row f1; needs a
    uint16 store and chunk-aligned z blocks), ``False`` = host gather / scatter through
    :func:`execute_worker`, ``None`` = the device path whenever it applies.

    ``device_codec``: ``True`` = the output chunks are encoded into Blosc-zstd frames on the GPU
    (``dsx_blosc_encode_device``: Huffman-coded literals, no matches -- about 1.1x the host writer's bytes, any c-blosc
    reader decodes them) and the host only writes finished bytes.  ``"runs"`` = the same with runs of equal bytes
    written as zstd matches (``DSX_ZENC_RUNS``): the empty high-byte planes cost a few dozen sequences instead of a bit
    per voxel, and a chunk is never larger than with ``True``; the pyramid rows of ``pyramid_group`` use the same mode.
    Any other string raises ``ValueError``; every other value counts by its truth.  Needs a Blosc-zstd output with byte
    shuffle and the device re-tiling path; anything else raises ``ValueError``.  Off by default.
    A Blosc-LZ4 output (``compressor`` a numcodecs config with ``cname`` ``"lz4"``: 2-byte elements, byte shuffle,
    ``blocksize`` 0) is written by the library's LZ4 encoder on either route: the I/O threads run its host build, and a
    true ``device_codec`` runs it on the GPU (``DSX_ZENC_LZ4``, ``LAST_RUN["device_codec_mode"] == "lz4"``) -- the same
    files.  ``"runs"`` on such an output raises ``ValueError`` before anything is created.

    ``device_decode``: ``True`` = the input chunks are decoded on the GPU (``dsx_blosc_decode_device``): the I/O
    threads only read the files, the compressed frames cross the host link, and a zstd decoder fills the input bricks.
    Frames the device does not take (other inner codecs, bit shuffle, split streams, zstd checksums) are decoded by the
    I/O threads as before.  ``"any"`` widens the device's share to what ``numcodecs.Blosc()`` writes by default and its
    common variants: LZ4 / LZ4HC inside, blocks split into a low-byte and a high-byte stream (LZ4 or zstd) and bit
    shuffle; blosclz, zlib and snappy inside, type sizes other than 2 and zstd checksums stay with the I/O threads.
    ``"full"`` adds blosclz and zlib inside Blosc frames and accepts a uint16 input whose compressor is plain ``zlib``
    (``csrc/dsx_inflate.h``; one wave inflates a stream serially: opt-in, not measured to be faster).  Any
    other string raises ``ValueError``; every other value counts by its truth.  ``LAST_RUN["decode_routes"]`` counts the
    chunks read over the z range by where they were decoded: ``{"device": n, "host": n, "fill": n}`` (``fill``: a
    missing file).  Needs a Blosc uint16 input and the device re-tiling path; anything else raises ``ValueError``.  Off
    by default; works with ``device_codec`` on or off.

    ``pyramid_group`` / ``n_levels`` (what ``destripe_zarr(fused_pyramid=True)`` is implemented with): with a group
    folder and ``n_levels > 1`` the pyramid levels ``1 .. n_levels - 1`` are written to ``<pyramid_group>/<i>`` in the
    same pass, from the filtered planes while they are in device memory (``dsx_pyramid_block_u16``) and through the same
    encode / download / write pipeline as level 0 -- the arrays, chunk files and voxels
    ``pyramid.write_pyramid_levels`` would produce from the finished level 0.  Every rank writes the levels of its own z
    range, which is then aligned to one chunk row of the deepest level (``output z chunk << (levels written - 1)``).
    Needs the device re-tiling path and z blocks that hold whole 2 x 2 x 2 windows of every level and fill whole chunk
    rows; anything else raises ``ValueError``.  Works with ``device_codec`` / ``device_decode`` on or off and with raw,
    zlib and Blosc outputs.  ``scale_factor`` ``(fz, fy, fx)``, 1 or 2 each and not all 1, is the window of the levels
    (an anisotropic volume reduces only its fine axes, e.g. ``(1, 2, 2)``); the z range of a rank is aligned to
    ``output z chunk * fz ** (levels written)`` planes, the plain output z chunk when z is not reduced, and z blocks hold
    whole ``fz``-windows of every level.  Anything else raises ``ValueError`` before anything is created.
    ``LAST_RUN["pyramid_scale"]`` is the scale of the levels written, ``None`` without a pyramid.

    ``streaks``: a dict ``{"sigma": (fg, bg), "level": 0, "wavelet": "db3", "crossover": 10, "threshold": -1,
    "route": "auto"}`` (defaults as in ``filtering.filter_streaks``; an unknown key raises ``TypeError``; a member of
    ``sigma`` may be ``None`` for a one-sided filter; optional keys ``"smoothing"``, the sigma 0 .. 2 of the gaussian
    over the blend weight, and ``"shading"``) runs the
    dual-band filter on every plane instead of the stripe filter: the device path plans a streaks engine, the host path
    (``device_retile=False`` or a geometry that is not chunk-aligned) calls ``filtering.destripe_streaks_planes``;
    everything around the filter -- re-tiling, codecs, pyramid, ranks -- is the same.  ``cells_config`` /
    ``no_cells_config`` may be ``None`` then.  Without ``"shading": True`` in the dict a ``shadow_correction``
    raises ``ValueError`` before anything is created; with it the flat / dark are resolved as for the stripe filter
    and the filter's result goes through ``flatfield_correction`` (no ``shadow_correction``: unshaded).
    ``LAST_RUN["filter"]`` is ``"stripes"`` or ``"streaks"``, ``LAST_RUN["streaks_route"]`` the route taken,
    ``LAST_RUN["streaks_smoothing"]`` the smoothing and ``LAST_RUN["streaks_shading"]`` whether a dark / flat step ran
    (all ``None`` for the stripe filter).

    ``histogram``: a zeroed ``np.int64[65536]``; this rank's share of the level-0 voxels it writes is added to it, one
    count per value -- what the display window of the OME-NGFF metadata is taken from
    (:func:`display_window_from_histogram`; ``zarr_destriper.py:722-726``).  On the device path the filtered planes of
    every block are counted where they lie, right behind the filter (``dsx_volhist_add_device``, one more read of them);
    the host path counts what it assigns.  ``LAST_RUN["histogram_voxels"]`` is the number added (``None`` without the
    option).  Anything but a C-contiguous ``int64`` array of 65 536 bins raises ``ValueError`` before anything is created.

    ``rotate``: ``True`` destripes a store whose stripes run down the columns -- every plane is filtered as
    ``np.rot90(F(np.rot90(x)), -1)``, ``F`` the filter without the option (either filter; a ``"rotate": True`` in the
    ``streaks`` dict asks for the same).  The engine turns the planes on the device inside its launch chain
    (``dsx_set_rotate``), so every route -- device re-tiling, device codecs, fused pyramid, histogram, the host path --
    runs as without it and sees planes in the store's orientation; the shading planes stay in that orientation too.
    Anything but a bool raises ``TypeError`` before anything is created.  ``LAST_RUN["rotate"]`` is the value used.

    ``lightsheet``: a dict ``{"percentile": .25, "artifact_length": 150, "background_window_size": 200,
    "lightsheet_vs_background": 2.0}`` (every key optional) runs the light-sheet background mode
    (``filtering.correct_lightsheet``) on every plane instead of the stripe filter: the device path plans a light-sheet
    engine, the host path calls ``filtering.correct_lightsheet_planes``; everything around the filter is the same and
    the configs may be ``None``.  An unknown key raises ``TypeError``; a bad value, a ``streaks`` dict or a
    ``shadow_correction`` given with it, or an input that is not uint16 raise ``ValueError``, all before anything is
    created.  ``LAST_RUN["filter"]`` is ``"lightsheet"`` then.

    ``projections``: a dict ``{"output": projections.VolumeProjections}`` or ``{"output": ..., "input": ...}``, built by
    the caller for the array's full ``zyx`` like ``histogram``; the maximum and sum projections of this rank's planes
    are added to it -- of the level-0 voxels it writes, and with ``"input"`` of the voxels it read (``projections.py``:
    MIPs, and the row sums before and after the filter whose ratio is the stripe gain).  On the device path
    ``dsx_project_u16_device`` runs right behind the filter on the planes where they lie, into device arrays of the
    rank's z range that are downloaded once after the last block; the host path projects what it reads and what it
    assigns (``dsx_project_u16_ref``).  No existing launch and no output byte changes.  ``LAST_RUN["projections"]`` is
    ``None``, ``"output"`` or ``"both"``, ``LAST_RUN["projection_planes"]`` the planes added (``None`` without the
    option).  A wrong key, type or shape and a store that is not uint16 raise ``ValueError`` before anything is created.

    ``digests=True``: level 0 and every fused pyramid level are created with a digest manifest (``.dsxdigest.json`` /
    ``.dsxdigest.bin`` next to the chunks, ``MiniZarrArray.create(digests=True)``; ``csrc/dsx_digest.h``): one record
    (valid voxels, their sum, their weighted sum mod 2^64) per chunk, of the voxels as they lie in device memory in chunk
    order behind ``planes_to_bricks`` / the pyramid kernel and in front of the encoder (``dsx_brick_digest_u16_device``,
    one more read of them); the records come back with the frame offsets (with the bricks when there is no device codec)
    and the writer of the block stores them at the block's own range of the file, so ranks write disjoint ranges and
    nothing is merged.  The host path records every chunk it writes with the host build.  No chunk file and no
    ``.zarray`` byte changes; off, no launch, allocation or file differs and a manifest left by an earlier run is
    removed.  ``integrity.verify_store`` reads a store back against it.  ``LAST_RUN["digests"]`` is the value used.
    """
    from . import projections as proj_mod
    from . import pyramid

    digests = bool(digests)
    rotate = engine_mod.rotate_flag(rotate)
    scale = pyramid.check_scale_factor(scale_factor)
    proj_mode = proj_mod.check_store_option(projections)

    logger = logger or logging.getLogger("dsx.zarr")
    if histogram is not None and not (isinstance(histogram, np.ndarray) and histogram.dtype == np.int64
                                      and histogram.shape == (engine_mod.VOLHIST_BINS,)
                                      and histogram.flags["C_CONTIGUOUS"] and histogram.flags["WRITEABLE"]):  # fmt: skip
        raise ValueError("histogram must be a writeable C-contiguous int64 array of {} bins".format(engine_mod.VOLHIST_BINS))
    if lightsheet is not None:
        lightsheet = fl.lightsheet_options(lightsheet, streaks, shadow_correction)
    if streaks is not None:
        streaks = fl.streaks_options(streaks)
        fl.streaks_shading(streaks, shadow_correction)
        rotate = rotate or streaks.get("rotate", False)
    codec_mode = output_codec_mode(device_codec, compressor)  # (a wrong mode fails before anything is created)
    device_codec = codec_mode is not None
    decode_mode = device_decode_mode(device_decode)
    if io_threads is None:
        io_threads = default_io_threads(world_size)
    src = MiniZarrArray.open(dataset_path)
    zyx = src.shape[-3:]
    if prediction_chunksize[1] < zyx[1] or prediction_chunksize[2] < zyx[2]:
        raise ValueError("blocks must cover whole planes: the stripe filter is a per-plane operation")
    if lightsheet is not None and src.dtype != np.uint16:
        raise ValueError("lightsheet: the store must be uint16, not {}".format(src.dtype))
    if proj_mode is not None:
        proj_mod.check_store_option(projections, zyx)
        if src.dtype != np.uint16:
            raise ValueError("projections: the store must be uint16, not {}".format(src.dtype))
    if streaks is not None:  # ("march" on an odd plane or another wavelet fails here, before anything is created)
        streaks["route"] = engine_mod.streaks_route(streaks["route"], zyx[1], zyx[2], streaks["wavelet"],
                                                    streaks["level"])  # fmt: skip
    out_shape = (1,) * (5 - len(src.shape)) + tuple(src.shape)
    out_chunks = tuple(output_chunks)[-len(out_shape):]
    fused = pyramid_group is not None and int(n_levels) > 1
    levels = pyramid.fused_levels(zyx, out_chunks, n_levels, scale) if fused else []
    lead = out_shape[:-3]
    level_arrays = [(os.path.join(str(pyramid_group), str(lv.level)), lead + lv.shape, (1,) * len(lead) + lv.chunks)
                    for lv in levels]  # fmt: skip
    if rank == 0:
        for path, shape, chunks in [(output_path, out_shape, out_chunks)] + level_arrays:
            MiniZarrArray.create(path, shape, chunks, np.uint16, compressor=compressor, dimension_separator="/",
                                 digests=digests)  # fmt: skip
    if group is not None and world_size > 1:
        group.barrier()

    def open_created(path, shape, chunks):
        for _ in range(1200):  # without a group: wait for rank 0's metadata of this geometry
            try:
                arr = MiniZarrArray.open(path)
                if arr.matches(shape, chunks, np.uint16, compressor) and (arr.digest_grid is not None) == digests:
                    return arr
            except (FileNotFoundError, ValueError):
                pass
            time.sleep(0.05)
        raise TimeoutError("rank {}: the output array {} was not created with shape {}".format(rank, path, shape))

    dst = open_created(output_path, out_shape, out_chunks)
    pyr_arrays = [open_created(*a) for a in level_arrays]
    if levels:  # every chunk of every level written by one rank: shards of whole chunk rows of the deepest level
        z0, z1 = pyramid.fused_z_range(zyx[0], world_size, rank, output_chunks[-3], levels, scale)
    else:
        z0, z1 = z_shard(zyx[0], world_size, rank, z_chunk=output_chunks[-3])
    dev = int(os.environ.get("LOCAL_RANK", rank)) if device is None else device
    LAST_RUN.update(rank=rank, world_size=world_size, z_range=(z0, z1), io_threads=int(io_threads), device=dev,
                    rotate=rotate, filter="lightsheet" if lightsheet is not None else "stripes" if streaks is None else "streaks",
                    streaks_route=None if streaks is None else streaks["route"],
                    streaks_smoothing=None if streaks is None else float(streaks.get("smoothing", 0.0)),
                    streaks_shading=None if streaks is None else bool(streaks.get("shading") and shadow_correction is not None))  # fmt: skip
    # dataset_name of the reference = the tile folder (X_..._Y_....zarr), also when level "0" is opened
    name = tile_name or os.path.basename(str(dataset_path).rstrip("/"))
    n_planes, t0 = 0, time.perf_counter()
    block_z = int(prediction_chunksize[0])
    can = z1 > z0 and _device_retile_ok(src, dst, zyx, block_z, z0, z1)
    if device_retile and not can:
        raise ValueError("device_retile needs a uint16 store, even planes and output-chunk-aligned z blocks")
    if device_codec:
        if not device_codec_output_ok(dst):
            raise ValueError("device_codec needs a Blosc-zstd or Blosc-LZ4 uint16 output with byte shuffle, not {!r}"
                             .format(dst.compressor))
        if not can or device_retile is False:
            raise ValueError("device_codec needs the device re-tiling path (a uint16 store, even planes and "
                             "output-chunk-aligned z blocks)")  # fmt: skip
    if device_decode:
        if not device_decode_input_ok(src, decode_mode):
            raise ValueError("device_decode needs a Blosc uint16 input, not {!r} {}".format(src.compressor, src.dtype))
        if not can or device_retile is False:
            raise ValueError("device_decode needs the device re-tiling path (a uint16 store, even planes and "
                             "output-chunk-aligned z blocks)")  # fmt: skip
    if levels and z1 > z0:
        if not can or device_retile is False:
            raise ValueError("fused_pyramid needs the device re-tiling path (a uint16 store, even planes and "
                             "output-chunk-aligned z blocks)")  # fmt: skip
        pyramid.fused_check_blocks(levels, block_z, scale)
    LAST_RUN.update(pyramid_scale=scale if levels else None)
    LAST_RUN.update(device_codec=device_codec, device_codec_mode=codec_mode, device_decode=bool(device_decode),
                    device_decode_mode=decode_mode, decode_routes=None, fused_pyramid=bool(levels), pyramid_levels=[lv.level for lv in levels])  # fmt: skip
    LAST_RUN["histogram_voxels"] = None if histogram is None else 0
    LAST_RUN.update(projections=proj_mode, projection_planes=None if proj_mode is None else 0, digests=digests)
    if can and device_retile is not False:
        if lightsheet is not None:
            eng = fl._lightsheet_engine(zyx[1:], lightsheet["percentile"], lightsheet["artifact_length"],
                                        lightsheet["background_window_size"], lightsheet["lightsheet_vs_background"],
                                        min(block_z, 64), dev, rotate)  # fmt: skip
        elif streaks is not None:
            flatfield, darkfield = fl._resolve_shading(shadow_correction, name.replace(".zarr", ""))
            eng = fl._streaks_engine(zyx[1:], *streaks["sigma"], streaks["level"], streaks["wavelet"], streaks["crossover"],
                                     streaks["threshold"], min(block_z, 64), dev, streaks["route"],
                                     streaks.get("smoothing", 0.0), flatfield, darkfield, rotate)  # fmt: skip
        else:
            flatfield, darkfield = fl._resolve_shading(shadow_correction, name.replace(".zarr", ""))
            eng = fl.get_engine(zyx[1:], cells_config, no_cells_config, 2500, flatfield, darkfield,
                                max_batch=min(block_z, 64), device=dev, rotate=rotate)  # fmt: skip
        blocks = _device_blocks(eng, src, dst, zyx, block_z, io_threads, "runs" if codec_mode == "runs" else device_codec,
                                device_decode, (levels, pyr_arrays) if levels else None, scale)  # fmt: skip
        blocks.histogram = histogram is not None
        blocks.enable_digests(digests)
        if histogram is not None:
            eng.volhist_reset()
        rank_zyx = (z1 - z0,) + tuple(zyx[1:])
        blocks.proj = None
        try:
            if proj_mode is not None:
                blocks.proj, blocks.proj_z0 = {}, z0
                for key in projections:
                    blocks.proj[key] = eng.alloc_projection(rank_zyx)
                blocks.proj_work = eng.alloc(engine_mod.project_work_bytes((min(block_z, z1 - z0),) + tuple(zyx[1:])))
            try:
                n_planes = blocks.run_range(z0, z1)
            finally:
                LAST_RUN["decode_routes"] = dict(blocks.timing["decode_routes"])
            eng.sync()
            if proj_mode is not None:  # one download per array, after the last block
                for key, bufs in blocks.proj.items():
                    projections[key].add_projected(z0, eng.projection_get(bufs, rank_zyx))
                LAST_RUN["projection_planes"] = z1 - z0
        finally:
            if blocks.proj is not None:
                for b in [b for bufs in blocks.proj.values() for b in bufs.values()] + [blocks.proj_work]:
                    if b is not None:
                        b.free()
                blocks.proj, blocks.proj_work = None, None
        if histogram is not None:
            counts = eng.volhist_get()
            histogram += counts
            LAST_RUN["histogram_voxels"] = int(counts.sum())
        dt = time.perf_counter() - t0
        logger.info("rank %d: %d planes z[%d:%d) in %.2f s (device re-tiling%s, overlapped; read %.2f s, write %.2f s)",
                    rank, n_planes, z0, z1, dt, (", device codec" + (" ({})".format(codec_mode) if codec_mode in ("runs", "lz4") else "") if device_codec else "")
                    + (", device decode ({})".format(decode_mode) if device_decode else "")
                    + (", pyramid levels 1..{} fused".format(len(levels)) if levels else ""), blocks.timing["read_s"],
                    blocks.timing["write_s"])  # fmt: skip
        return n_planes, dt
    for sc, internal in iter_blocks(zyx, prediction_chunksize, (z0, z1)):
        lead = (0,) * (len(src.shape) - 3)
        block = src[lead + sc]
        data = block[np.newaxis].astype(np.float32) if block.dtype != np.uint16 else block[np.newaxis]
        written = execute_worker(data, sc, internal, cells_config, no_cells_config, (0, 0, 0), dst, shadow_correction,
                                 name, logger, device=dev, streaks=streaks, rotate=rotate, lightsheet=lightsheet)  # fmt: skip
        if histogram is not None:
            counts = np.bincount(written.ravel(), minlength=engine_mod.VOLHIST_BINS)
            histogram += counts
            LAST_RUN["histogram_voxels"] += int(counts.sum())
        if proj_mode is not None:
            projections["output"].add(sc[0].start, written.reshape((-1,) + written.shape[-2:]))
            if "input" in projections:
                projections["input"].add(sc[0].start, block)
            LAST_RUN["projection_planes"] += block.shape[0]
        n_planes += block.shape[0]
    dt = time.perf_counter() - t0
    logger.info("rank %d: %d planes z[%d:%d) in %.2f s", rank, n_planes, z0, z1, dt)
    return n_planes, dt


def default_io_threads(world_size=1):
    """Codec threads of ONE rank: the cores this process may run on, shared among the ranks of the node.

    The chunk codecs are the bottleneck of this path (zstd level 5 runs at ~0.7 GB/s per core, the filter at
    > 500 GB/s), so a rank takes every core it can -- as the reference's ``CO_CPUS`` consumers do
    (``zarr_destriper.py:1091, 1138``) -- but eight ranks on one node must not take every core eight times:
    the budget is ``cores // LOCAL_WORLD_SIZE`` (``LOCAL_WORLD_SIZE`` as set by ``torchrun``, else ``world_size``:
    one node), at least 2, at most 64.
    """
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 8
    local = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world_size) or 1))
    return max(2, min(cores // local, 64))


def _cpu_limit():
    """``utils.get_code_ocean_cpu_limit`` (``utils/utils.py:197-226``): ``CO_CPUS``, else the cores of this process."""
    co_cpus = os.environ.get("CO_CPUS")
    if co_cpus:
        return int(co_cpus)
    try:
        return len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        return os.cpu_count() or 1


def _group_broadcasts(group, world_size):
    """True when ``group`` can hand planes from rank 0 to the other ranks (a ``distributed.RankGroup``) and there is
    somebody to hand them to -- or the group holds a communicator anyway (one rank with ``DSX_FORCE_COMM=1``: rehearsal)."""
    return (hasattr(group, "broadcast_array") and hasattr(group, "broadcast_json")
            and (world_size > 1 or bool(getattr(group, "active", False))))


def _broadcast_planes(group, rank, world_size, read):
    """``read()`` (a dict of arrays / ``None``) runs on rank 0 only; every rank gets the arrays.

    ``group`` with ``broadcast_array`` / ``broadcast_json`` (``distributed.RankGroup``): the planes travel as ONE
    collective per array -- RCCL over xGMI, or the rendezvous directory on the host transport -- instead of every rank
    reading the same TIFF files (the reference reads them once per tile, ``zarr_destriper.py:1099-1130, 1249``).  An
    exception of rank 0's ``read`` is re-raised on EVERY rank (nobody is left waiting in a collective).  Any other
    group (or a single rank): every rank reads for itself.
    """
    if not _group_broadcasts(group, world_size):
        return read()
    status, planes = {"ok": True}, {}
    if rank == 0:
        try:
            planes = read()
            status["keys"] = {k: (None if v is None else [np.asarray(v).dtype.str, list(np.asarray(v).shape)])
                              for k, v in planes.items()}  # fmt: skip
        except Exception as e:  # noqa: BLE001 - handed to every rank below
            status = {"ok": False, "type": type(e).__name__, "error": str(e)}
    status = group.broadcast_json(status, root=0)
    if not status["ok"]:
        exc = {"FileNotFoundError": FileNotFoundError, "ValueError": ValueError, "KeyError": KeyError}.get(
            status["type"], RuntimeError)
        raise exc(status["error"])
    out = {}
    for k in sorted(status["keys"]):
        meta = status["keys"][k]
        if meta is None:
            out[k] = None
            continue
        src = np.ascontiguousarray(planes[k]) if rank == 0 else None
        out[k] = group.broadcast_array(src, np.dtype(meta[0]), tuple(meta[1]), root=0)
    return out


def compute_pyramid(data, n_lvls, scale_axis, chunks="auto", device=0, engine=None):
    """``zarr_destriper.py:365-407`` (re-exported under the reference's module name; the kernel side is ``pyramid.py``)."""
    from . import pyramid

    return pyramid.compute_pyramid(data, n_lvls, scale_axis, chunks=chunks, device=device, engine=engine)


# ---------------------------------------------------------------------------------------------
# OME-NGFF metadata of the group (reference ``zarr_destriper.py:410-674``) and its display window
# ---------------------------------------------------------------------------------------------
REFERENCE_DISPLAY_WINDOW = (0.0, 350.0)  # what the reference writes for every SmartSPIM channel (``:722-726``)
REFERENCE_CHANNEL_COLOR = 0x690AFE  # (``:737``)


def _get_axes_5d(time_unit="millisecond", space_unit="micrometer"):
    """The five OME-NGFF axes t, c, z, y, x (reference ``zarr_destriper.py:507-528``): the channel axis has no unit."""
    axes = [{"name": "t", "type": "time", "unit": str(time_unit)}, {"name": "c", "type": "channel"}]
    axes += [{"name": name, "type": "space", "unit": str(space_unit)} for name in "zyx"]
    return axes


def _compute_scales(scale_num_levels, scale_factor, pixelsizes, chunks, data_shape, translation=None):
    """Per-level coordinate transformations and chunk options (reference ``zarr_destriper.py:410-504``).

    Level 0 has the voxel size ``pixelsizes`` (z, y, x) behind two unit axes; every further level multiplies the spatial
    scales by ``scale_factor`` and divides the spatial shape by it, rounding up; the chunk option of a level is
    ``chunks`` clamped to the level's spatial shape, ``(1, 1)`` in front.  ``translation`` (five numbers) is appended to
    every level's list.  Returns ``(transforms, chunk options)``, one entry per level (at least one)."""
    transforms, chunk_sizes = [], []
    scale = [float(p) if isinstance(p, (int, np.integer)) else p for p in tuple(pixelsizes)[:3]]
    shape = [int(n) for n in tuple(data_shape)[2:5]]
    for level in range(max(1, int(scale_num_levels))):
        if level:
            scale = [s * f for s, f in zip(scale, scale_factor)]
            shape = [int(np.ceil(n / f)) for n, f in zip(shape, scale_factor)]
        entry = [{"type": "scale", "scale": [1.0, 1.0] + list(scale)}]
        if translation is not None:
            entry.append({"type": "translation", "translation": translation})
        transforms.append(entry)
        chunk_sizes.append({"chunks": (1, 1) + tuple(min(n, int(c)) for n, c in zip(shape, tuple(chunks)[2:5]))})
    return transforms, chunk_sizes


def _build_ome(data_shape, image_name, channel_names=None, channel_colors=None, channel_minmax=None,
               channel_startend=None):  # fmt: skip
    """The ``omero`` block of the group attributes (reference ``zarr_destriper.py:531-597``): one channel entry per
    element of axis 1 of ``data_shape`` (t, c, z, y, x) -- label, colour as six hex digits, the value range ``min`` /
    ``max`` and the display window ``start`` / ``end`` as floats -- and the middle plane as the default z.  Defaults:
    names ``Channel:<image_name>:<i>``, colours ``i``, range ``(0.0, 1.0)``, window = range."""
    n_channels = int(data_shape[1])
    if channel_names is None:
        channel_names = ["Channel:{}:{}".format(image_name, i) for i in range(n_channels)]
    if channel_colors is None:
        channel_colors = list(range(n_channels))
    if channel_minmax is None:
        channel_minmax = [(0.0, 1.0)] * n_channels
    if channel_startend is None:
        channel_startend = channel_minmax
    channels = []
    for i in range(n_channels):
        lo, hi = channel_minmax[i]
        start, end = channel_startend[i]
        channels.append({
            "active": True,
            "coefficient": 1,
            "color": "{:06x}".format(channel_colors[i]),
            "family": "linear",
            "inverted": False,
            "label": channel_names[i],
            "window": {"end": float(end), "max": float(hi), "min": float(lo), "start": float(start)},
        })  # fmt: skip
    return {
        "id": 1,
        "name": image_name,
        "version": "0.4",
        "channels": channels,
        "rdefs": {"defaultT": 0, "defaultZ": int(data_shape[2]) // 2, "model": "color"},
    }


def _validate_coordinate_transformations(ndim, n_levels, transforms):
    """What ``ome_zarr.format.FormatV04.validate_coordinate_transformations`` checks (the reference calls it at
    ``zarr_destriper.py:664-666``), as ``ValueError``: one list per level, each with exactly one ``scale`` of ``ndim``
    numbers in first place and at most one ``translation`` of ``ndim`` numbers after it."""
    if len(transforms) != n_levels:
        raise ValueError("coordinate transformations: {} lists for {} levels".format(len(transforms), n_levels))
    for level, entry in enumerate(transforms):
        if not isinstance(entry, (list, tuple)):
            raise ValueError("coordinate transformations of level {}: not a list".format(level))
        types = [t.get("type") if isinstance(t, dict) else None for t in entry]
        if types.count("scale") != 1 or types[0] != "scale":
            raise ValueError("coordinate transformations of level {}: exactly one scale, in first place, not {}"
                             .format(level, types))  # fmt: skip
        if types[1:] not in ([], ["translation"]):
            raise ValueError("coordinate transformations of level {}: only one translation may follow the scale, not {}"
                             .format(level, types[1:]))  # fmt: skip
        for t in entry:
            values = t.get(t["type"])
            if not isinstance(values, (list, tuple)) or len(values) != ndim:
                raise ValueError("coordinate transformations of level {}: {} needs {} numbers, got {!r}"
                                 .format(level, t["type"], ndim, values))  # fmt: skip
            if not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in values):
                raise ValueError("coordinate transformations of level {}: {} holds a non-number: {!r}"
                                 .format(level, t["type"], values))  # fmt: skip


def _write_json_atomic(path, obj):
    """``obj`` as JSON under ``path``, through a temporary file and a rename (as ``MiniZarrArray.create`` writes
    ``.zarray``): a reader sees the file whole or not at all."""
    tmp = "{}.tmp.{}".format(path, os.getpid())
    with open(tmp, "w") as f:
        json.dump(obj, f, indent=4)
    os.replace(tmp, path)


def _plain_json(obj):
    """NumPy scalars / arrays / tuples -> what ``json`` writes."""
    if isinstance(obj, dict):
        return {str(k): _plain_json(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain_json(v) for v in obj]
    if isinstance(obj, np.ndarray):
        return _plain_json(obj.tolist())
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def write_ome_ngff_metadata(group, arr, image_name, n_lvls, scale_factors, voxel_size, channel_names=None,
                            channel_colors=None, channel_minmax=None, channel_startend=None, metadata=None):  # fmt: skip
    """The OME-NGFF 0.4 metadata of a multiscale group (reference ``zarr_destriper.py:600-674``).

    ``group``: the group folder (a path, or anything with ``.path``); ``arr``: level 0 -- anything with ``.shape``
    (t, c, z, y, x) and ``.chunks`` or ``.chunksize`` (a :class:`MiniZarrArray`).  Written into the folder, each file
    through a temporary file and a rename:

    * ``.zgroup``: ``{"zarr_format": 2}``;
    * ``.zattrs``: ``"omero"`` = :func:`_build_ome`; ``"multiscales"`` = one entry ``{"version": "0.4", "name": "/",
      "axes": the five axes, "datasets": [{"path": "<i>", "coordinateTransformations": [scale (, translation)]}, ...],
      **metadata}`` for the levels ``0 .. n_lvls - 1`` (:func:`_compute_scales` from ``voxel_size`` = z, y, x and
      ``scale_factors``).  Keys of an existing ``.zattrs`` other than these two are kept.

    ``"name": "/"`` is what ome-zarr-py's ``write_multiscales_metadata`` is understood to put for a root group
    (``group.name``); no interpreter this was written with has ome-zarr installed, so this one value is NOT verified
    against the library.  The checks of its ``validate_coordinate_transformations`` are restated and raise
    ``ValueError`` before anything is written."""
    group_path = str(getattr(group, "path", group))
    shape = tuple(int(n) for n in arr.shape)
    if len(shape) != 5:
        raise ValueError("write_ome_ngff_metadata: level 0 must be 5-D (t, c, z, y, x), not {}".format(shape))
    chunks = getattr(arr, "chunks", None)
    if chunks is None:
        chunks = arr.chunksize
    n_lvls = int(n_lvls)
    ome = _build_ome(shape, image_name, channel_names=channel_names, channel_colors=channel_colors,
                     channel_minmax=channel_minmax, channel_startend=channel_startend)  # fmt: skip
    transforms, _ = _compute_scales(n_lvls, scale_factors, voxel_size, tuple(chunks), shape, None)
    _validate_coordinate_transformations(len(shape), n_lvls, transforms)
    datasets = [{"path": str(i), "coordinateTransformations": t} for i, t in enumerate(transforms)]
    multiscale = {"version": "0.4", "name": "/", "axes": _get_axes_5d(), "datasets": datasets}
    multiscale.update(metadata or {})
    attrs_path = os.path.join(group_path, ".zattrs")
    attrs = read_json_as_dict(attrs_path)
    attrs["omero"] = ome
    attrs["multiscales"] = [multiscale]
    attrs = _plain_json(attrs)
    json.dumps(attrs)  # (anything json cannot write fails here, before a file exists)
    os.makedirs(group_path, exist_ok=True)
    _write_json_atomic(os.path.join(group_path, ".zgroup"), {"zarr_format": 2})
    _write_json_atomic(attrs_path, attrs)


def display_window_from_histogram(hist, percentiles=(0.1, 95.0)):
    """Display window ``(start, end)`` of a volume from its exact histogram ``hist`` (one count per integer value): the
    ``da.percentile(image_data, (0.1, 95))`` the reference names as the ideal and does not compute
    (``zarr_destriper.py:722-726``).

    For each ``q`` of ``percentiles`` the data value ``np.percentile(volume, q, method="lower")`` returns: the element
    of the sorted volume at index ``floor((N - 1) * (q / 100.0))`` (NumPy's own float64 arithmetic), i.e. the smallest
    ``v`` with ``cumsum(hist)[v]`` above that index.  Floats; ``end = max(end, start + 1.0)``, so a constant volume
    still gives a window a viewer can use.  An all-zero histogram raises ``ValueError``."""
    h = np.asarray(hist)
    if h.ndim != 1 or h.size == 0 or not np.issubdtype(h.dtype, np.integer):
        raise ValueError("display_window_from_histogram: hist is a 1-D array of integer counts")
    if (h < 0).any():
        raise ValueError("display_window_from_histogram: negative counts")
    qs = tuple(percentiles)
    if len(qs) != 2 or not all(0.0 <= float(q) <= 100.0 for q in qs):
        raise ValueError("display_window_from_histogram: percentiles are two numbers in [0, 100], not {!r}".format(percentiles))
    cum = np.cumsum(h.astype(np.int64))
    total = int(cum[-1])
    if total == 0:
        raise ValueError("display_window_from_histogram: the histogram is empty")
    values = []
    for q in qs:
        index = int(np.floor((total - 1) * (np.float64(q) / 100.0)))
        values.append(float(np.searchsorted(cum, index, side="right")))
    start, end = values
    return start, max(end, start + 1.0)


def _resolve_display_window(display_window, histogram):
    """The ``(start, end)`` pair a ``display_window`` option selects (:func:`compute_multiscale`); ``ValueError`` for
    anything it does not take."""
    if display_window is None:
        return REFERENCE_DISPLAY_WINDOW
    if isinstance(display_window, str):
        if display_window != "percentile":
            raise ValueError("display_window is None, a (start, end) pair or \"percentile\", not {!r}".format(display_window))
        if histogram is None:
            raise ValueError("display_window=\"percentile\" needs the histogram of the volume")
        return display_window_from_histogram(histogram)
    try:
        start, end = display_window
        if isinstance(start, (str, bool)) or isinstance(end, (str, bool)):
            raise TypeError
        pair = (float(start), float(end))
    except (TypeError, ValueError):
        raise ValueError("display_window is None, a (start, end) pair or \"percentile\", not {!r}"
                         .format(display_window)) from None  # fmt: skip
    if not all(np.isfinite(pair)):
        raise ValueError("display_window: the pair must be finite, not {!r}".format(display_window))
    return pair


def _check_ome_options(ome_metadata, display_window, histogram, voxel_size, image_name):
    """The option rules of :func:`compute_multiscale` (``ValueError`` before anything is written); returns the window
    to write, or ``None`` with the metadata off."""
    if not ome_metadata:
        if display_window is not None or histogram is not None:
            raise ValueError("display_window / histogram need ome_metadata=True")
        return None
    try:
        sizes = [float(v) for v in voxel_size]
    except (TypeError, ValueError):
        raise ValueError("ome_metadata: voxel_size is three positive numbers (z, y, x), not {!r}".format(voxel_size)) from None
    if len(sizes) != 3 or not all(np.isfinite(v) and v > 0 for v in sizes):
        raise ValueError("ome_metadata: voxel_size is three positive numbers (z, y, x), not {!r}".format(voxel_size))
    if not isinstance(image_name, str):
        raise ValueError("ome_metadata: image_name is a string, not {!r}".format(image_name))
    return _resolve_display_window(display_window, histogram)


def _write_group_metadata(group_path, level0, image_name, n_levels, scale_factor, voxel_size, window):
    """``write_ome_ngff_metadata`` with the reference's values (``zarr_destriper.py:713-741``) and the window."""
    arr = level0 if hasattr(level0, "shape") else MiniZarrArray.open(str(level0))
    n_channels = int(arr.shape[1]) if len(arr.shape) == 5 else 1
    info = np.iinfo(np.uint16)
    write_ome_ngff_metadata(
        group=group_path,
        arr=arr,
        image_name=image_name,
        n_lvls=n_levels,
        scale_factors=scale_factor,
        voxel_size=voxel_size,
        channel_names=[image_name],
        channel_colors=[REFERENCE_CHANNEL_COLOR],
        channel_minmax=[(int(info.min), int(info.max))] * n_channels,
        channel_startend=[tuple(window)] * n_channels,
        metadata=None,
    )


def compute_multiscale(
    output_zarr,
    zarr_group,
    scale_factor,
    n_workers,
    voxel_size,
    image_name,
    n_levels=3,
    threads_per_worker=1,
    *,
    chunks=(1, 1, 64, 128, 128),
    compressor="blosc",
    device=0,
    slab_planes=None,
    pipelined=False,
    device_codec=False,
    device_decode=False,
    io_threads=None,
    ome_metadata=False,
    display_window=None,
    histogram=None,
    digests=False,
):
    """``compute_multiscale`` of the reference (``zarr_destriper.py:677-794``) with its signature.

    ``output_zarr``: level 0 (a :class:`MiniZarrArray` or its path); ``zarr_group``: the group folder the levels
    ``1 .. n_levels - 1`` are written into (a path, or anything with ``.path``).  ``n_workers`` /
    ``threads_per_worker`` sized the reference's dask ``LocalCluster`` (``:689-697``): accepted, not used -- one HIP
    kernel per level replaces the cluster.  ``voxel_size`` (z, y, x) / ``image_name`` feed the OME-NGFF metadata
    (``:728-742``), which is written with ``ome_metadata=True`` only.  Returns the shapes of the written levels.

    ``ome_metadata=True``: once the levels are written, ``.zgroup`` and ``.zattrs`` of the group
    (:func:`write_ome_ngff_metadata`) with the reference's values (``:713-741``): channel name ``image_name``, colour
    ``690afe``, range ``(0, 65535)``.  ``display_window`` is the channel's ``start`` / ``end``: ``None`` = the
    reference's ``(0.0, 350.0)``, a pair of numbers = that pair, ``"percentile"`` = the 0.1 % / 95 % points of
    ``histogram`` (``np.int64[65536]`` counts of level 0, :func:`display_window_from_histogram`; this call does not
    compute one itself).  ``voxel_size`` must then be three positive numbers and ``image_name`` a string;
    ``display_window`` / ``histogram`` without ``ome_metadata``, ``"percentile"`` without ``histogram`` and any other
    value raise ``ValueError`` before anything is written.  Off by default: no file is added to the group.

    ``pipelined=True``: the same stores from one software-pipelined pass over level 0 -- level 0 is read by ``io_threads``
    native threads into pinned staging, every level comes from the block where it lies in chunk order
    (``dsx_pyramid_bricks_u16``), no level is read back (``pyramid.write_pyramid_levels``; ``slab_planes`` is ignored).
    ``device_decode`` / ``device_codec`` (as in :func:`destripe_zarr_store`: ``False``, ``True``, ``"any"``, ``"full"`` / ``"runs"``)
    then decode level 0 and encode the levels on the GPU; without ``pipelined`` they raise ``ValueError``.
    ``pyramid.LAST_PYRAMID`` holds what the call did.

    ``scale_factor`` ``(fz, fy, fx)``: 1 or 2 per axis, not all 1 -- ``[2, 2, 2]`` in production (``:1176``), e.g.
    ``[1, 2, 2]`` for a volume whose z step is coarser than its pixel; level ``l`` is ``previous // factor`` per axis.
    Every route takes it; anything else raises ``ValueError`` before anything is written.

    ``digests=True``: every level written gets a digest manifest (``pyramid.write_pyramid_levels(digests=True)``; on the
    pipelined route the records are taken on the device from the finished chunk rows, on the slab route by the host
    build as the chunks are written).  ``pyramid.LAST_PYRAMID["digests"]`` says what ran.
    """
    from . import pyramid

    del n_workers, threads_per_worker
    pyramid.check_scale_factor(scale_factor)  # (a scale the kernels do not take fails before anything is written)
    window = _check_ome_options(ome_metadata, display_window, histogram, voxel_size, image_name)
    level0 = getattr(output_zarr, "path", output_zarr)
    group_path = getattr(zarr_group, "path", zarr_group)
    if window is not None and len(MiniZarrArray.open(str(level0)).shape) != 5:
        raise ValueError("ome_metadata: level 0 must be 5-D (t, c, z, y, x)")
    shapes = pyramid.write_pyramid_levels(str(level0), str(group_path), scale_factor=tuple(scale_factor), n_levels=n_levels,
                                          chunks=chunks, compressor=compressor, device=device, slab_planes=slab_planes,
                                          pipelined=pipelined, device_codec=device_codec, device_decode=device_decode,
                                          io_threads=io_threads, digests=bool(digests))  # fmt: skip
    if window is not None:
        _write_group_metadata(str(group_path), str(level0), image_name, n_levels, scale_factor, voxel_size, window)
    return shapes


def destripe_zarr(
    dataset_path,
    multiscale,
    output_destriped_zarr,
    prediction_chunksize,
    target_size_mb,
    n_workers,
    batch_size,
    super_chunksize,
    results_folder,
    derivatives_path,
    xyz_resolution,
    parameters,
    flatfield=None,
    lazy_callback_fn=None,
    *,
    rank=0,
    world_size=1,
    device=None,
    compressor="blosc",
    output_chunks=(1, 1, 64, 128, 128),
    n_levels=3,
    logger=None,
    device_retile=None,
    io_threads=None,
    group=None,
    device_codec=False,
    device_decode=False,
    fused_pyramid=False,
    pipelined_pyramid=False,
    streaks=None,
    ome_metadata=False,
    display_window=None,
    rotate=False,
    lightsheet=None,
    scale_factor=None,
    qc_projections=None,
    digests=False,
    verify=False,
):
    """``destripe_zarr`` of the reference (``zarr_destriper.py:909-1211``) with its 14 parameters, on the GPU chunk map.

    What the reference does with them, and what happens here:

    * ``dataset_path`` / ``multiscale``: the tile ``.zarr`` and the level to process (``:1027-1035``) -- level
      ``<dataset_path>/<multiscale>`` is opened (or ``dataset_path`` itself when it already is an array).
    * ``output_destriped_zarr``: a group of that name is created with array ``0`` in it (``:1060-1075``: uint16, chunks
      ``(1, 1, 64, 128, 128)``, Blosc-zstd level 3 with byte shuffle, ``"/"`` separator, always anew) and levels
      ``1 .. 2`` of the pyramid next to it (``:1176-1192``, ``n_levels=3``).
    * ``prediction_chunksize``: z-block of the chunk map; blocks must cover whole planes (the filter is per plane).
    * ``parameters``: ``cells_config`` / ``no_cells_config`` (``:972-973``, ``KeyError`` without them).
    * ``derivatives_path`` / ``flatfield``: the ``shadow_correction`` dict is built as ``:1095-1130`` does
      (:func:`load_shadow_correction`: ``DarkMaster_cropped.tif``, retrospective flat if given, else the
      normalised microscope flats + tile config); no derivatives folder and no flat = no shading correction.
    * ``n_workers``: ``ValueError`` when above the CPU limit, like ``:977-978``; otherwise unused -- so are
      ``target_size_mb``, ``batch_size``, ``super_chunksize`` (sizing of the reference's data loader, ``:1041-1057``):
      the loader is out of scope.  ``results_folder`` (log file and resource plots, ``:980,
      1202-1211``): no log file or resource plot is written; with ``qc_projections`` the QC files of the tile go there.  ``xyz_resolution`` (OME-NGFF voxel size, ``:1181-1185``) is used with ``ome_metadata=True``.
    * ``lazy_callback_fn``: applied by the reference's loader to the lazy array (``:1052``); ``None`` in production
      (``:1266``).  Anything else raises ``NotImplementedError`` -- silently skipping a transform would change the data.

    Keyword-only extras (the engine's): ``rank`` / ``world_size`` / ``group`` (one process per GPU, chunk-aligned
    z-ranges; with a ``distributed.RankGroup`` rank 0 alone reads the dark plane and broadcasts it), ``device``,
    ``compressor`` / ``output_chunks`` of the output, ``n_levels``, ``device_retile``, ``io_threads``, ``device_codec``, ``device_decode``
    (level 0 encoded / decoded on the GPU, :func:`destripe_zarr_store`; ``device_codec="runs"`` = with run matches), ``fused_pyramid`` (levels ``1 .. n_levels - 1``
    are written by every rank in the level-0 pass, from the filtered planes in device memory, instead of by
    :func:`compute_multiscale` on rank 0 afterwards; same stores; z shards of ``output z chunk << (levels - 1)`` planes),
    ``pipelined_pyramid`` (rank 0's :func:`compute_multiscale` call runs with ``pipelined=True``, this call's
    ``device_codec`` and ``io_threads``, and this call's ``device_decode`` when the output is Blosc -- level 0 is this
    run's own output; same stores; ``ValueError`` together with ``fused_pyramid``), ``streaks`` (the dict of
    :func:`destripe_zarr_store`: the dual-band filter instead of the stripe filter; ``parameters`` need no configs then,
    and, unless the dict says ``"shading": True``, a derivatives folder that exists or a ``flatfield`` raises
    ``ValueError`` before anything is created; with it they are read as for the stripe filter), ``ome_metadata`` / ``display_window`` (rank 0 writes the group's ``.zgroup`` and
    OME-NGFF ``.zattrs`` once the levels are written -- inside :func:`compute_multiscale`, or itself on the
    ``fused_pyramid`` route; the same file on every route.  ``xyz_resolution`` is the voxel size, handed on as
    ``[z, y, x]``; ``display_window`` as in :func:`compute_multiscale`, except that ``"percentile"`` needs nothing from
    the caller: every rank counts the voxels it writes (``destripe_zarr_store(histogram=...)``), ``group.sum_counts``
    adds the ranks' counts after the barrier, and rank 0 raises ``RuntimeError`` unless they add up to the voxels of
    level 0.  ``"percentile"`` with ``world_size > 1`` and a group without ``sum_counts`` raises ``ValueError`` before
    anything is created.  ``LAST_RUN["display_window"]`` is the pair written, or ``None``), ``rotate`` (vertical stripes:
    :func:`destripe_zarr_store`; a bool, ``TypeError`` before anything is created otherwise), ``lightsheet`` (the dict
    of :func:`destripe_zarr_store`: the light-sheet background mode instead of the stripe filter; ``parameters`` need no
    configs then; together with ``streaks``, a ``flatfield`` or a derivatives folder that exists it raises
    ``ValueError`` before anything is created -- the mode has no dark / flat step), ``scale_factor`` (``(fz, fy, fx)`` of
    the pyramid, 1 or 2 each and not all 1; ``None`` = the reference's ``[2, 2, 2]``, ``:1176``; it goes to the fused
    route, to rank 0's :func:`compute_multiscale` and to the metadata; anything else raises ``ValueError`` before
    anything is created.  ``LAST_RUN["pyramid_scale"]`` is the scale used), ``qc_projections`` (``None``, ``"output"``
    or ``"both"``: every rank collects the maximum and sum projections of the planes it writes -- with ``"both"`` also
    of the planes it read -- in the pass itself (``destripe_zarr_store(projections=...)``), ``group.reduce_array``
    merges the ranks' arrays after the barrier, and rank 0 writes ``<tile>_projections.npz`` and the three
    ``<tile>_mip_{z,y,x}.tif`` into ``results_folder`` (``projections.write_qc``; ``"both"`` adds the input's arrays and
    the stripe gain).  Any other value, and ``world_size > 1`` with a group without ``reduce_array``, raise
    ``ValueError`` before anything is created), ``digests`` (every array of the tile keeps a digest manifest:
    :func:`destripe_zarr_store` for level 0 and the fused levels, :func:`compute_multiscale` for the others) and
    ``verify`` (implies ``digests``: once the last level is written rank 0 reads the whole tile back with
    ``integrity.verify_store`` -- the call's ``device_decode`` and ``io_threads`` -- and raises ``ValueError`` listing
    every chunk that does not hold what was written; ``LAST_RUN["verify"]`` is the report, ``None`` without the option).
    Returns ``(planes processed by this rank, seconds)``.
    """
    from . import projections as proj_mod
    from . import pyramid

    digests = bool(digests) or bool(verify)
    rotate = engine_mod.rotate_flag(rotate)
    proj_mod.check_qc_mode(qc_projections)
    if qc_projections is not None and world_size > 1 and not hasattr(group, "reduce_array"):
        raise ValueError("qc_projections with world_size > 1 needs a group with reduce_array (distributed.RankGroup): "
                         "the ranks' projections must be merged")  # fmt: skip
    scale_factor = list(pyramid.check_scale_factor([2, 2, 2] if scale_factor is None else scale_factor))
    output_codec_mode(device_codec, compressor)  # (a wrong string or mode fails before anything is written)
    device_decode_mode(device_decode)
    if fused_pyramid and pipelined_pyramid:
        raise ValueError("fused_pyramid and pipelined_pyramid are two routes to the same pyramid: choose one")
    percentile = isinstance(display_window, str) and display_window == "percentile"
    try:  # (x, y, z) -> the [z, y, x] the metadata wants; anything else is left for the check below to refuse
        voxel_size = [xyz_resolution[-1], xyz_resolution[-2], xyz_resolution[-3]]
    except (TypeError, IndexError, KeyError):
        voxel_size = None
    fixed_window = _check_ome_options(ome_metadata, None if percentile and ome_metadata else display_window, None,
                                      voxel_size, Path(output_destriped_zarr).name)  # fmt: skip
    if percentile and world_size > 1 and not hasattr(group, "sum_counts"):
        raise ValueError("display_window=\"percentile\" with world_size > 1 needs a group with sum_counts "
                         "(distributed.RankGroup): the ranks' voxel counts must be added")  # fmt: skip
    histogram = np.zeros(engine_mod.VOLHIST_BINS, np.int64) if percentile else None
    if lightsheet is not None:
        shaded = flatfield is not None or os.path.exists(Path(derivatives_path))
        lightsheet = fl.lightsheet_options(lightsheet, streaks, True if shaded else None)
        no_cells_config, cells_config = parameters.get("no_cells_config"), parameters.get("cells_config")
    elif streaks is not None:
        streaks = fl.streaks_options(streaks)
        if not streaks.get("shading") and (flatfield is not None or os.path.exists(Path(derivatives_path))):
            raise ValueError("streaks: the dual-band filter has no dark / flat step without 'shading': True; give no "
                             "flatfield and no derivatives folder")  # fmt: skip
        no_cells_config, cells_config = parameters.get("no_cells_config"), parameters.get("cells_config")
    else:
        no_cells_config = parameters["no_cells_config"]
        cells_config = parameters["cells_config"]
    co_cpus = _cpu_limit()
    if n_workers > co_cpus:
        raise ValueError(f"Provided workers {n_workers} > current workers {co_cpus}")
    if lazy_callback_fn is not None:
        raise NotImplementedError("lazy_callback_fn: the GPU chunk map reads the store as it is (production passes None)")
    del target_size_mb, batch_size, super_chunksize
    logger = logger or logging.getLogger("dsx.zarr")
    logger.info(f"Processing dataset {dataset_path}")
    dataset_path = Path(dataset_path)
    output_destriped_zarr = Path(output_destriped_zarr)
    level = dataset_path.joinpath(str(multiscale))
    src = level if level.joinpath(".zarray").exists() else dataset_path
    dataset_name = output_destriped_zarr.name
    derivatives_path = Path(derivatives_path)

    def read_shading():
        sc = load_shadow_correction(derivatives_path, output_destriped_zarr, flatfield, logger)
        return {"darkfield": sc["darkfield"], "microscope_flats": None if sc["retrospective"] else sc["flatfield"],
                "tile_config": sc["tile_config"]}  # fmt: skip

    if lightsheet is not None or (streaks is not None and not streaks.get("shading")):
        shadow_correction = {"flatfield": None, "darkfield": None}
    elif _group_broadcasts(group, world_size):
        tile_config = {}

        def read_planes():
            got = read_shading()
            tile_config["v"] = got.pop("tile_config")
            return got

        planes = _broadcast_planes(group, rank, world_size, read_planes)
        tc = group.broadcast_json(tile_config.get("v"), root=0)
        shadow_correction = {
            "retrospective": flatfield is not None,
            "flatfield": flatfield if flatfield is not None else planes["microscope_flats"],
            "darkfield": planes["darkfield"],
            "tile_config": tc,
        }
    else:
        shadow_correction = load_shadow_correction(derivatives_path, output_destriped_zarr, flatfield, logger)
    if shadow_correction["flatfield"] is None:
        if shadow_correction["darkfield"] is not None:
            # the reference would hand flatfield=None to flatfield_correction and fail inside NumPy (filtering.py:371-391)
            raise ValueError("a darkfield without a flatfield: give `flatfield` or put FlatReal*.tif + metadata.json into "
                             f"{derivatives_path}")  # fmt: skip
        shadow_correction = None
    elif shadow_correction["darkfield"] is None:
        # flatfield_correction dereferences the dark plane (filtering.py:371-377): nothing to correct with
        raise ValueError(f"No darkfield for the shading correction: {derivatives_path} does not exist")
    level0 = output_destriped_zarr.joinpath("0")
    qc = None
    if qc_projections is not None:  # (a volume the projections do not take fails here, before anything is created)
        src_zyx = MiniZarrArray.open(str(src)).shape[-3:]
        qc = {key: proj_mod.VolumeProjections(src_zyx) for key in (("output", "input") if qc_projections == "both" else ("output",))}
    n_planes, seconds = destripe_zarr_store(
        str(src),
        str(level0),
        cells_config,
        no_cells_config,
        shadow_correction=shadow_correction,
        prediction_chunksize=tuple(prediction_chunksize),
        output_chunks=output_chunks,
        rank=rank,
        world_size=world_size,
        device=device,
        compressor=compressor,
        logger=logger,
        device_retile=device_retile,
        io_threads=io_threads,
        tile_name=dataset_name,
        group=group,
        device_codec=device_codec,
        device_decode=device_decode,
        pyramid_group=str(output_destriped_zarr) if fused_pyramid else None,
        n_levels=n_levels if fused_pyramid else 1,
        scale_factor=scale_factor,
        streaks=streaks,
        histogram=histogram,
        rotate=rotate,
        lightsheet=lightsheet,
        projections=qc,
        digests=digests,
    )
    if group is not None and world_size > 1:
        group.barrier()  # level 0 of this tile is complete on every rank: the pyramid may read it
    if qc is not None:
        for p in qc.values():
            p.merge(group if world_size > 1 else None)
        if rank == 0:
            proj_mod.write_qc(results_folder, dataset_name.replace(".zarr", ""), qc["output"], qc.get("input"),
                              rotate=bool(LAST_RUN.get("rotate", rotate)))  # fmt: skip
    window, ome_kw = fixed_window, {}
    if percentile:
        total = group.sum_counts(histogram) if world_size > 1 else histogram
        voxels = int(np.prod(MiniZarrArray.open(str(level0)).shape[-3:]))
        if rank == 0 and int(total.sum()) != voxels:  # padded, skipped or twice-counted voxels would move the percentiles
            raise RuntimeError("display_window=\"percentile\": the ranks counted {} voxels, level 0 holds {}"
                               .format(int(total.sum()), voxels))  # fmt: skip
        window = display_window_from_histogram(total)
        ome_kw = dict(ome_metadata=True, display_window="percentile", histogram=total)
    elif ome_metadata:
        ome_kw = dict(ome_metadata=True, display_window=display_window)
    LAST_RUN["display_window"] = window
    LAST_RUN["pyramid_scale"] = tuple(scale_factor) if n_levels > 1 else None
    if rank == 0 and ome_metadata and (fused_pyramid or n_levels <= 1):  # compute_multiscale is not called: the same file
        _write_group_metadata(str(output_destriped_zarr), str(level0), dataset_name, n_levels, scale_factor, voxel_size,
                              window)  # fmt: skip
    if rank == 0 and n_levels > 1 and not fused_pyramid:
        dev = int(os.environ.get("LOCAL_RANK", rank)) if device is None else device
        pipelined_kw = {}
        if pipelined_pyramid:
            out_is_blosc = (MiniZarrArray._compressor_meta(compressor) or {}).get("id") == "blosc"  # level 0 = our output
            pipelined_kw = dict(pipelined=True, device_codec=device_codec, io_threads=io_threads,
                                device_decode=device_decode if out_is_blosc else False)  # fmt: skip
        t0 = time.perf_counter()
        compute_multiscale(
            output_zarr=str(level0),
            zarr_group=str(output_destriped_zarr),
            scale_factor=scale_factor,
            n_workers=co_cpus,
            voxel_size=[xyz_resolution[-1], xyz_resolution[-2], xyz_resolution[-3]] if xyz_resolution is not None else None,
            image_name=dataset_name,
            n_levels=n_levels,
            threads_per_worker=1,
            chunks=output_chunks,
            compressor=compressor,
            device=dev,
            digests=digests,
            **pipelined_kw,
            **ome_kw,
        )
        logger.info(f"Processing multiscale time: {time.perf_counter() - t0} seconds")
    LAST_RUN["verify"] = None
    if verify and rank == 0:  # every level of the tile is written (fused: by every rank, before the barrier above)
        from . import integrity

        dev = int(os.environ.get("LOCAL_RANK", rank)) if device is None else device
        report = integrity.verify_store(str(output_destriped_zarr), device_decode=device_decode, io_threads=io_threads,
                                        device=dev)  # fmt: skip
        LAST_RUN["verify"] = report
        if report["bad"]:
            raise ValueError("verify: {} of {} chunks of {} do not hold what was written: {}".format(
                len(report["bad"]), report["chunks"], output_destriped_zarr, integrity.format_bad(report)))  # fmt: skip
    logger.info(f"Processing destripe flatfield time: {seconds} seconds")
    return n_planes, seconds


def destripe_channel(
    zarr_dataset_path,
    derivatives_path,
    channel_name,
    results_folder,
    xyz_resolution,
    estimated_channel_flats,
    laser_tiles,
    parameters,
    *,
    multiscale="0",
    prediction_chunksize=(64, 1600, 2000),
    output_chunks=(1, 1, 64, 128, 128),
    rank=0,
    world_size=1,
    device=None,
    compressor="blosc",
    n_levels=3,
    logger=None,
    group=None,
    io_threads=None,
    device_retile=None,
    device_codec=False,
    device_decode=False,
    fused_pyramid=False,
    pipelined_pyramid=False,
    ome_metadata=False,
    display_window=None,
    streaks=None,
    rotate=False,
    scale_factor=None,
    qc_projections=None,
    digests=False,
    verify=False,
):
    """``destripe_channel`` of the reference (``zarr_destriper.py:1214-1267``), same eight parameters (the reference's
    caller passes them by keyword, ``run_capsule.py:394-403``), wired to the GPU chunk map.

    For every ``<channel>/<tile>.zarr``: pick the retrospective flat of the laser side the tile belongs to
    (``laser_tiles`` = ``{side: [tile stems]}``, ``ValueError`` for a tile in neither, ``:1239-1247``), read it
    (``:1249``) and call :func:`destripe_zarr` with the reference's arguments (``:1252-1267``):
    ``<results>/destriped_data/<channel>/<tile>.zarr/0`` plus pyramid levels ``1 .. n_levels - 1``.
    ``xyz_resolution`` is the voxel size of the OME-NGFF metadata: handed on, and written with ``ome_metadata=True``
    (``ome_metadata`` / ``display_window`` go to every tile's :func:`destripe_zarr`; with ``"percentile"`` each tile
    gets the window of its own voxels).
    Returns ``{tile name: planes processed by this rank}``.

    Keyword-only extras: ``rank`` / ``world_size`` / ``group`` / ``device`` (one process per GPU), output codec and
    chunks, ``multiscale`` (the reference hard-codes ``"0"``), ``prediction_chunksize`` (the reference hard-codes the
    production tile, ``(64, 1600, 2000)``), ``io_threads``, ``device_retile``, ``device_codec``, ``device_decode``, ``fused_pyramid``, ``pipelined_pyramid`` (:func:`destripe_zarr`).  ``world_size > 1`` needs ``group`` (anything with
    ``barrier()``): the pyramid of a tile may only be computed once EVERY rank has written its z-range.  With a
    ``distributed.RankGroup`` rank 0 alone reads the flat and dark planes of a tile and broadcasts them (RCCL).
    ``streaks``: the dict of :func:`destripe_zarr_store`, handed to every tile's :func:`destripe_zarr`.  Every tile
    comes with its retrospective flat here, so the dict must say ``"shading": True`` (``ValueError`` before anything is
    created otherwise).  ``rotate``: vertical stripes, handed to every tile's :func:`destripe_zarr` (a bool,
    ``TypeError`` before anything is created otherwise).  ``scale_factor``: the pyramid's ``(fz, fy, fx)``, handed to
    every tile's :func:`destripe_zarr` (``None`` = ``[2, 2, 2]``; ``ValueError`` before anything is created otherwise).
    ``qc_projections``: ``None``, ``"output"`` or ``"both"``, handed to every tile's :func:`destripe_zarr`, which leaves
    the tile's QC files in ``results_folder`` (``ValueError`` before anything is created for any other value, and with
    ``world_size > 1`` for a group without ``reduce_array``).  ``digests`` / ``verify``: handed to every tile's
    :func:`destripe_zarr` (a digest manifest per array; read the tile back against it once it is written).
    """
    from . import projections as proj_mod
    from . import pyramid

    rotate = engine_mod.rotate_flag(rotate)
    proj_mod.check_qc_mode(qc_projections)
    if qc_projections is not None and world_size > 1 and not hasattr(group, "reduce_array"):
        raise ValueError("qc_projections with world_size > 1 needs a group with reduce_array (distributed.RankGroup): "
                         "the ranks' projections must be merged")  # fmt: skip
    if scale_factor is not None:
        pyramid.check_scale_factor(scale_factor)
    if world_size > 1 and group is None:
        raise ValueError("destripe_channel with world_size > 1 needs a group to order the pyramid after all ranks")
    if streaks is not None and not fl.streaks_options(streaks).get("shading"):
        raise ValueError("streaks: the dual-band filter has no dark / flat step without 'shading': True, and "
                         "destripe_channel hands every tile its flat")  # fmt: skip
    output_codec_mode(device_codec, compressor)  # (a wrong string or mode fails before anything is written)
    device_decode_mode(device_decode)
    if fused_pyramid and pipelined_pyramid:
        raise ValueError("fused_pyramid and pipelined_pyramid are two routes to the same pyramid: choose one")
    if not ome_metadata and display_window is not None:
        raise ValueError("display_window needs ome_metadata=True")
    if (isinstance(display_window, str) and display_window == "percentile" and world_size > 1
            and not hasattr(group, "sum_counts")):  # fmt: skip
        raise ValueError("display_window=\"percentile\" with world_size > 1 needs a group with sum_counts "
                         "(distributed.RankGroup): the ranks' voxel counts must be added")  # fmt: skip
    logger = logger or logging.getLogger("dsx.zarr")
    zarr_dataset_path, results_folder = Path(zarr_dataset_path), Path(results_folder)
    channel_dataset = zarr_dataset_path.joinpath(channel_name)
    destriped_data_folder = results_folder.joinpath("destriped_data")
    os.makedirs(destriped_data_folder, exist_ok=True)
    done = {}
    for tile_path in sorted(channel_dataset.glob("*.zarr")):
        output_folder = destriped_data_folder.joinpath(f"{channel_name}/{tile_path.name}")
        logger.info(f"Processing {tile_path} - writing to: {output_folder} - derivatives: {derivatives_path}")
        flatfield_path = None
        tile_stem = tile_path.stem.rsplit(".", 1)[0]
        for side, tiles in laser_tiles.items():
            if tile_stem in tiles:
                flatfield_path = estimated_channel_flats[int(side)]
                break
        if flatfield_path is None:
            raise ValueError(f"Tile {tile_path} not found in {laser_tiles}")
        flatfield = _broadcast_planes(group, rank, world_size, lambda: {"flat": tif.imread(str(flatfield_path))})["flat"]
        n, _ = destripe_zarr(
            dataset_path=tile_path,
            multiscale=multiscale,
            output_destriped_zarr=output_folder,
            prediction_chunksize=prediction_chunksize,
            target_size_mb=3072,
            n_workers=0,
            batch_size=1,
            super_chunksize=(384, 1600, 2000),
            results_folder=results_folder,
            derivatives_path=derivatives_path,
            xyz_resolution=xyz_resolution,
            parameters=parameters,
            flatfield=flatfield,
            lazy_callback_fn=None,
            rank=rank,
            world_size=world_size,
            device=device,
            compressor=compressor,
            output_chunks=output_chunks,
            n_levels=n_levels,
            logger=logger,
            io_threads=io_threads,
            device_retile=device_retile,
            group=group,
            device_codec=device_codec,
            device_decode=device_decode,
            fused_pyramid=fused_pyramid,
            pipelined_pyramid=pipelined_pyramid,
            ome_metadata=ome_metadata,
            display_window=display_window,
            streaks=streaks,
            rotate=rotate,
            scale_factor=scale_factor,
            qc_projections=qc_projections,
            digests=digests,
            verify=verify,
        )
        done[tile_path.name] = n
    return done
