"""ctypes binding of ``libdsx_hip.so`` (C ABI in ``include/dsx.h``).

No GPU array library is involved: device memory, copies, streams and timing all go through the
C ABI.  The engine has NO CPU fallback -- if the library is missing or no MI355X is visible the
constructor raises :class:`DsxError`.
"""

import ctypes
import math
import os

import numpy as np

from . import wavelets

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSX_LIB overrides the library path (A/B runs of two builds inside one GPU session)
LIB_PATH = os.environ.get("DSX_LIB") or os.path.join(_HERE, "_lib", "libdsx_hip.so")

DSX_U16, DSX_F32 = 0, 1
DSX_WAVELET_DB3 = 3
DSX_WAVELET_BANK = 0  # filter bank handed over with dsx_set_wavelet
STAGE_APPROX, STAGE_DETAIL = 0, 1
STREAM_COMPUTE, STREAM_UPLOAD, STREAM_DOWNLOAD = 0, 1, 2

# Blosc block tasks of the device decoder (csrc/dsx_zdec_task.h DecTask): kinds, the un-shuffle flag, routes per chunk
TASK_FILL, TASK_COPY, TASK_STORED, TASK_ZSTD, TASK_LZ4 = 0, 1, 2, 3, 4
TASK_ZLIB, TASK_BLOSCLZ = 5, 6  # (one zlib stream, one blosclz stream)
TASK_SHUFFLE, TASK_SPLIT, TASK_BITSHUFFLE = 0x100, 0x200, 0x400  # (split streams, bit un-shuffle)
ZDEC_ZSTD, ZDEC_ANY, ZDEC_ALL = 0, 1, 3  # (2 stays refused) DSX_ZDEC_*: what dsx_io_read_frames_ex routes to the device
ROUTE_DEVICE, ROUTE_HOST, ROUTE_FILL = 0, 1, 2
TASK_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<u4"), ("dst_len", "<u4"), ("kind", "<u4"),
                       ("chunk", "<u4")])  # fmt: skip

COMM_ID_BYTES = 128
VOLHIST_BINS = 65536  # one bin per uint16 value (dsx_volhist_*)
# one record of dsx_brick_digest_u16_*: the valid voxels of a chunk, their sum and their weighted sum (mod 2^64)
DIGEST_DTYPE = np.dtype([("count", "<u8"), ("sum", "<u8"), ("wsum", "<u8")])
DIGEST_MAX_BRICK = 1 << 31  # voxels per brick
STACK_RANK_MAX_PLANES = 512  # planes, quantiles and elements per plane of one dsx_stack_rank_u16_* call
STACK_RANK_MAX_QUANTILES = 4
STACK_RANK_MAX_ELEMS = (1 << 31) - 1
GAUSS_MAX_SIGMA = 64.0  # dsx_gauss_smooth_f64_* / dsx_flat_finish_*: radius int(4 sigma + 0.5) <= 256
GAUSS_MAX_RADIUS = 256
FLAT_FINISH_MAX_ELEMS = (1 << 31) - 1  # H * W of one plane
PROJECT_MAX_EXTENT = 65536  # rows, columns, and planes of one call (dsx_project_*: the uint32 sums)
# the six projections of a uint16 volume [Z, H, W] (dsx_projection, in the order of its members): name, dtype, the two
# axes of zyx that are left
PROJECTION_ARRAYS = (("max_z", np.uint16, (1, 2)), ("sum_z", np.uint64, (1, 2)), ("max_y", np.uint16, (0, 2)),
                     ("sum_y", np.uint32, (0, 2)), ("max_x", np.uint16, (0, 1)), ("sum_x", np.uint32, (0, 1)))  # fmt: skip
_ERRORS = {-1: "DSX_EINVAL", -2: "DSX_ENOPLAN", -3: "DSX_EHIP", -4: "DSX_ENOMEM", -5: "DSX_ELIMIT",
           -6: "DSX_ECOMM", -7: "DSX_EIO", -8: "DSX_EVALUE"}  # fmt: skip

# every symbol include/dsx.h declares (tests/test_host_native.py checks the list against the header)
EXPORTED_SYMBOLS = [
    "dsx_init", "dsx_destroy", "dsx_last_error", "dsx_device_count", "dsx_plan", "dsx_plan_info", "dsx_set_wavelet", "dsx_graph_stats",
    "dsx_row_pack_launches",
    "dsx_set_shading_device", "dsx_constants_device", "dsx_run_host", "dsx_run_device", "dsx_sync",
    "dsx_malloc", "dsx_free", "dsx_memcpy_h2d", "dsx_memcpy_d2h", "dsx_memcpy_d2d",
    "dsx_timer_start", "dsx_timer_stop", "dsx_profile_enable", "dsx_profile_read",
    "dsx_get_stats", "dsx_get_thresholds", "dsx_get_level", "dsx_set_stop_after", "dsx_set_stack_mode",
    "dsx_bricks_to_planes_u16", "dsx_planes_to_bricks_u16", "dsx_downsample2_u16",
    "dsx_flatfield_correction", "dsx_flatfield_correction_rows", "dsx_foreground_background",
    "dsx_comm_unique_id", "dsx_comm_init", "dsx_comm_destroy", "dsx_comm_broadcast", "dsx_comm_allreduce_f64",
    "dsx_malloc_host", "dsx_free_host", "dsx_memcpy_h2d_async", "dsx_memcpy_d2h_async",
    "dsx_stream_wait", "dsx_stream_sync", "dsx_event_record", "dsx_event_sync",
    "dsx_io_read_chunks", "dsx_io_write_chunks", "dsx_io_write_chunks_blosc", "dsx_blosc_decode", "dsx_blosc_encode",
    "dsx_png_unfilter", "dsx_plan_streaks", "dsx_plan_streaks_ex", "dsx_get_streaks_threshold",
    "dsx_blosc_encode_device", "dsx_blosc_encode_ref", "dsx_blosc_encode_device_ex", "dsx_blosc_encode_ref_ex",
    "dsx_io_read_frames", "dsx_io_read_frames_ex", "dsx_blosc_decode_device", "dsx_blosc_decode_ref",
    "dsx_io_read_zlib_chunks", "dsx_io_write_chunks_blosc_lz4", "dsx_blosc_encode_lz4",
    "dsx_pyramid_work_bytes", "dsx_pyramid_block_u16", "dsx_pyramid_block_ref",
    "dsx_pyramid_bricks_u16", "dsx_pyramid_bricks_ref",
    "dsx_downsample_u16", "dsx_pyramid_work_bytes_scale", "dsx_pyramid_block_scale_u16", "dsx_pyramid_block_scale_ref",
    "dsx_pyramid_bricks_scale_u16", "dsx_pyramid_bricks_scale_ref",
    "dsx_volhist_reset", "dsx_volhist_add_device", "dsx_volhist_get", "dsx_volhist_ref",
    "dsx_stack_rank_u16_device", "dsx_stack_rank_u16_ref",
    "dsx_gauss_smooth_f64_device", "dsx_gauss_smooth_f64_ref",
    "dsx_flat_finish_work_bytes", "dsx_flat_finish_device", "dsx_flat_finish_ref",
    "dsx_project_work_bytes", "dsx_project_u16_device", "dsx_project_u16_ref",
    "dsx_brick_digest_u16_device", "dsx_brick_digest_u16_ref",
    "dsx_plan_streaks_opts", "dsx_streaks_blend_ref",
    "dsx_set_rotate", "dsx_rot90_device", "dsx_rot90_ref",
    "dsx_plan_lightsheet", "dsx_lightsheet_ref", "dsx_get_lightsheet_planes",
]  # fmt: skip


def frame_tasks_per_chunk(chunk_bytes):
    """Most tasks one chunk may take (``csrc/dsx_io.h frame_tasks_per_chunk``)."""
    return int(chunk_bytes) // 8192 + 1


def decode_task(src, dst, src_len, dst_len, kind, chunk=0):
    """One task as a ``TASK_DTYPE`` array of length 1 (tests, tools)."""
    t = np.zeros(1, TASK_DTYPE)
    t[0] = (src, dst, src_len, dst_len, kind, chunk)
    return t


class DsxError(RuntimeError):
    """Error reported by the HIP engine (code + message of ``dsx_last_error``)."""

    def __init__(self, code, message):
        super().__init__("{} ({}): {}".format(_ERRORS.get(code, "DSX_E?"), code, message))
        self.code = code
        self.message = message


class _Cfg(ctypes.Structure):
    _fields_ = [
        ("wavelet", ctypes.c_int32),
        ("level", ctypes.c_int32),
        ("sigma", ctypes.c_float),
        ("max_threshold", ctypes.c_float),
    ]


class _StreaksCfg(ctypes.Structure):
    _fields_ = [
        ("wavelet", ctypes.c_int32),
        ("level", ctypes.c_int32),
        ("sigma_fg", ctypes.c_float),
        ("sigma_bg", ctypes.c_float),
        ("crossover", ctypes.c_float),
        ("otsu", ctypes.c_int32),
        ("threshold", ctypes.c_float),
    ]


class _StreaksOpts(ctypes.Structure):
    _fields_ = [
        ("bands", ctypes.c_int32),
        ("smoothing", ctypes.c_float),
        ("flat", ctypes.c_void_p),
        ("dark", ctypes.c_void_p),
        ("dark_h", ctypes.c_int32),
        ("dark_w", ctypes.c_int32),
    ]


class _PyramidLevel(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("cz", "cy", "cx", "rows", "z0", "zero")]


class _Projection(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in PROJECTION_ARRAYS]


class _PlanInfo(ctypes.Structure):
    _fields_ = [
        ("height", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("out_height", ctypes.c_int32),
        ("out_width", ctypes.c_int32),
        ("levels", ctypes.c_int32),
        ("level_h", ctypes.c_int32 * 16),
        ("level_w", ctypes.c_int32 * 16),
        ("fft_len", ctypes.c_int32 * 16),
        ("fft_halo", ctypes.c_int32 * 16),
        ("max_batch", ctypes.c_int32),
        ("workspace_bytes", ctypes.c_uint64),
    ]


_lib = None


def load_library(path=None):
    """Load ``libdsx_hip.so``; raises ``DsxError`` if it has not been built (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise DsxError(
            -3,
            "{} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the destripe engine has no CPU fallback)".format(p),
        )
    lib = ctypes.CDLL(p)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)
    lib.dsx_init.argtypes = [i32, ctypes.POINTER(vp)]
    lib.dsx_destroy.argtypes = [vp]
    lib.dsx_destroy.restype = None
    lib.dsx_last_error.argtypes = [vp]
    lib.dsx_last_error.restype = ctypes.c_char_p
    lib.dsx_device_count.argtypes = []
    lib.dsx_plan.argtypes = [vp, i32, i32, i32, ctypes.POINTER(_Cfg), ctypes.POINTER(_Cfg),
                             ctypes.c_double, vp, vp, i32, i32]  # fmt: skip
    lib.dsx_plan_info.argtypes = [vp, ctypes.POINTER(_PlanInfo)]
    lib.dsx_set_shading_device.argtypes = [vp, vp, vp, i32, i32]
    lib.dsx_constants_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_run_host.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    lib.dsx_run_device.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    lib.dsx_sync.argtypes = [vp]
    lib.dsx_malloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.dsx_free.argtypes = [vp, vp]
    lib.dsx_memcpy_h2d.argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.dsx_memcpy_d2h.argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.dsx_memcpy_d2d.argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.dsx_timer_start.argtypes = [vp]
    lib.dsx_timer_stop.argtypes = [vp, f32p]
    lib.dsx_profile_enable.argtypes = [vp, i32]
    lib.dsx_profile_read.argtypes = [vp, i32, f32p, ctypes.POINTER(ctypes.c_int32),
                                     ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i32)]  # fmt: skip
    lib.dsx_get_stats.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]  # fmt: skip
    lib.dsx_get_thresholds.argtypes = [vp, i32, i32, f32p, f32p]
    lib.dsx_get_level.argtypes = [vp, i32, i32, i32, vp]
    lib.dsx_set_stop_after.argtypes = [vp, i32]
    lib.dsx_set_stack_mode.argtypes = [vp, i32]
    lib.dsx_graph_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.dsx_row_pack_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dsx_set_wavelet.argtypes = [vp] +[ctypes.POINTER(ctypes.c_double)] * 4 + [i32]
    lib.dsx_bricks_to_planes_u16.argtypes = [vp, vp, vp] + [i32] * 7
    lib.dsx_planes_to_bricks_u16.argtypes = [vp, vp, vp] + [i32] * 7
    lib.dsx_downsample2_u16.argtypes = [vp, vp, vp, i32, i32, i32]
    lib.dsx_foreground_background.argtypes = [vp, vp, i32, ctypes.c_size_t, ctypes.c_float,
                                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), vp]  # fmt: skip
    lib.dsx_flatfield_correction.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, ctypes.c_float, vp]
    lib.dsx_flatfield_correction_rows.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, ctypes.c_float, vp, vp]
    lib.dsx_comm_unique_id.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    lib.dsx_comm_init.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, i32, i32]
    lib.dsx_comm_destroy.argtypes = [vp]
    lib.dsx_comm_broadcast.argtypes = [vp, vp, ctypes.c_size_t, i32]
    lib.dsx_comm_allreduce_f64.argtypes = [vp, ctypes.POINTER(ctypes.c_double), i32, i32]
    lib.dsx_malloc_host.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.dsx_free_host.argtypes = [vp, vp]
    lib.dsx_memcpy_h2d_async.argtypes = [vp, vp, vp, ctypes.c_size_t, i32]
    lib.dsx_memcpy_d2h_async.argtypes = [vp, vp, vp, ctypes.c_size_t, i32]
    lib.dsx_stream_wait.argtypes = [vp, i32, i32]
    lib.dsx_stream_sync.argtypes = [vp, i32]
    lib.dsx_event_record.argtypes = [vp, i32, i32]
    lib.dsx_event_sync.argtypes = [vp, i32]
    lib.dsx_io_read_chunks.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                       ctypes.POINTER(ctypes.c_size_t), i32, i32, i32, ctypes.c_uint16]  # fmt: skip
    lib.dsx_io_write_chunks.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                        ctypes.POINTER(ctypes.c_size_t), i32, i32, i32]  # fmt: skip
    lib.dsx_io_write_chunks_blosc.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                              ctypes.POINTER(ctypes.c_size_t), i32, i32, i32, i32, i32]  # fmt: skip
    lib.dsx_io_write_chunks_blosc_lz4.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp),
                                                  ctypes.POINTER(ctypes.c_size_t), i32, i32, i32]  # fmt: skip
    lib.dsx_blosc_encode_lz4.argtypes = [vp, ctypes.c_size_t, i32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_png_unfilter.argtypes = [vp, i32, i32, i32]
    lib.dsx_plan_streaks.argtypes = [vp, i32, i32, i32, ctypes.POINTER(_StreaksCfg)]
    lib.dsx_plan_streaks_ex.argtypes = [vp, i32, i32, i32, ctypes.POINTER(_StreaksCfg), i32]
    lib.dsx_get_streaks_threshold.argtypes = [vp, i32, f32p]
    lib.dsx_plan_streaks_opts.argtypes = [vp, i32, i32, i32, ctypes.POINTER(_StreaksCfg), i32,
                                          ctypes.POINTER(_StreaksOpts)]  # fmt: skip
    lib.dsx_streaks_blend_ref.argtypes = [vp, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float,
                                          ctypes.POINTER(_StreaksOpts), vp, i32]  # fmt: skip
    lib.dsx_set_rotate.argtypes = [vp, i32]
    lib.dsx_rot90_device.argtypes = [vp, vp, vp] + [i32] * 5
    lib.dsx_rot90_ref.argtypes = [vp, vp] + [i32] * 5
    lib.dsx_blosc_decode.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t]
    lib.dsx_blosc_encode.argtypes = [vp, ctypes.c_size_t, i32, i32, i32, vp, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]  # fmt: skip
    lib.dsx_blosc_encode_device.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, i32, vp, vp]
    lib.dsx_blosc_encode_ref.argtypes = [vp, i32, ctypes.c_size_t, i32, i32, vp, vp]
    lib.dsx_blosc_encode_device_ex.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, i32, vp, vp, i32]
    lib.dsx_blosc_encode_ref_ex.argtypes = [vp, i32, ctypes.c_size_t, i32, i32, vp, vp, i32]
    lib.dsx_io_read_frames.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32, ctypes.c_size_t, i32, ctypes.c_uint16,
                                       vp, ctypes.c_size_t, vp, i32, ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.POINTER(i32), vp]  # fmt: skip
    lib.dsx_io_read_frames_ex.argtypes = lib.dsx_io_read_frames.argtypes + [i32]
    lib.dsx_io_read_zlib_chunks.argtypes = lib.dsx_io_read_frames.argtypes
    lib.dsx_blosc_decode_device.argtypes = [vp, vp, ctypes.c_size_t, vp, i32, vp, ctypes.c_size_t, vp]
    lib.dsx_blosc_decode_ref.argtypes = [vp, ctypes.c_size_t, vp, i32, vp, ctypes.c_size_t, vp]
    lib.dsx_pyramid_work_bytes.argtypes = [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_pyramid_block_u16.argtypes = [vp, vp, i32, i32, i32, i32, ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp),
                                          vp, ctypes.c_size_t]  # fmt: skip
    lib.dsx_pyramid_block_ref.argtypes = [vp, i32, i32, i32, i32, ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp)]
    lib.dsx_pyramid_bricks_u16.argtypes = [vp, vp] + [i32] * 7 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp), vp,
                                                                  ctypes.c_size_t]  # fmt: skip
    lib.dsx_pyramid_bricks_ref.argtypes = [vp] + [i32] * 7 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp)]
    # the same with a scale factor per axis (fz, fy, fx in front of n_levels)
    lib.dsx_downsample_u16.argtypes = [vp, vp, vp] + [i32] * 6
    lib.dsx_pyramid_work_bytes_scale.argtypes = [i32] * 7 + [ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_pyramid_block_scale_u16.argtypes = [vp, vp] + [i32] * 7 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp),
                                                                       vp, ctypes.c_size_t]  # fmt: skip
    lib.dsx_pyramid_block_scale_ref.argtypes = [vp] + [i32] * 7 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp)]
    lib.dsx_pyramid_bricks_scale_u16.argtypes = [vp, vp] + [i32] * 10 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp),
                                                                         vp, ctypes.c_size_t]  # fmt: skip
    lib.dsx_pyramid_bricks_scale_ref.argtypes = [vp] + [i32] * 10 + [ctypes.POINTER(_PyramidLevel), ctypes.POINTER(vp)]
    lib.dsx_volhist_reset.argtypes = [vp]
    lib.dsx_volhist_add_device.argtypes = [vp, vp, ctypes.c_size_t]
    lib.dsx_volhist_get.argtypes = [vp, vp]
    lib.dsx_volhist_ref.argtypes = [vp, ctypes.c_size_t, vp]
    i32p = ctypes.POINTER(ctypes.c_int)
    lib.dsx_stack_rank_u16_device.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, i32, i32p, i32, vp, vp]
    lib.dsx_stack_rank_u16_ref.argtypes = [vp, i32, ctypes.c_size_t, i32, i32, i32p, i32, vp, vp]
    f64, f64p = ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    lib.dsx_gauss_smooth_f64_device.argtypes = [vp, vp, i32, i32, f64p, i32, vp, vp]
    lib.dsx_gauss_smooth_f64_ref.argtypes = [vp, i32, i32, f64p, i32, vp, vp]
    lib.dsx_flat_finish_work_bytes.argtypes = [i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_flat_finish_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, f64p, i32, f64, vp, vp, vp]
    lib.dsx_flat_finish_ref.argtypes = [vp, vp, i32, i32, i32, i32, i32, f64p, i32, f64, vp, vp]
    lib.dsx_project_work_bytes.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.dsx_project_u16_device.argtypes = [vp, vp, i32, i32, i32, ctypes.POINTER(_Projection), i32, i32, vp]
    lib.dsx_project_u16_ref.argtypes = [vp, i32, i32, i32, ctypes.POINTER(_Projection), i32, i32]
    lib.dsx_brick_digest_u16_device.argtypes = [vp, vp] + [i32] * 9 + [vp, i32]
    lib.dsx_brick_digest_u16_ref.argtypes = [vp] + [i32] * 9 + [vp]
    f64 = ctypes.c_double
    lib.dsx_plan_lightsheet.argtypes = [vp, i32, i32, i32, f64, i32, i32, f64, vp, vp]
    lib.dsx_lightsheet_ref.argtypes = [vp, i32, i32, f64, i32, i32, f64, vp, vp, vp, vp, vp, i32]
    lib.dsx_get_lightsheet_planes.argtypes = [vp, i32, vp, vp]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("dsx_destroy", "dsx_last_error"):
            fn.restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


STREAKS_ROUTES = {"generic": 0, "march": 1}  # DSX_STREAKS_GENERIC, DSX_STREAKS_MARCH
STREAKS_BANDS = {"both": 0, "fg": 1, "bg": 2}  # DSX_STREAKS_BANDS_BOTH, _FG, _BG
STREAKS_MAX_SMOOTHING = 2.0


def streaks_smoothing(smoothing):
    """``smoothing`` of the blend weight as a float: 0 (none) or ``0 < s <= 2``; ``ValueError`` for anything else."""
    try:
        s = float(smoothing)
    except (TypeError, ValueError):
        raise ValueError("smoothing must be 0 or a value in (0, 2], not {!r}".format(smoothing))
    if not (0.0 <= s <= STREAKS_MAX_SMOOTHING):  # (nan fails both comparisons)
        raise ValueError("smoothing must be 0 or a value in (0, 2], not {!r}".format(smoothing))
    return s


def rotate_flag(rotate):
    """``rotate`` as the C ABI takes it; anything but a ``bool`` is a ``TypeError`` (raised before any device call)."""
    if not isinstance(rotate, (bool, np.bool_)):
        raise TypeError("rotate must be True or False, not {!r}".format(rotate))
    return bool(rotate)


LIGHTSHEET_DEFAULTS = {"percentile": 0.25, "artifact_length": 150, "background_window_size": 200,
                       "lightsheet_vs_background": 2.0}  # fmt: skip
LIGHTSHEET_MAX_ARTIFACT = 1024  # kLsMaxA
LIGHTSHEET_MAX_WINDOW = 255  # kLsMaxB: B * B fits a 16-bit count


def lightsheet_params(percentile=0.25, artifact_length=150, background_window_size=200, lightsheet_vs_background=2.0):
    """The four parameters of the light-sheet background mode as ``(p, A, B, lam)``, checked: ``ValueError`` for a value
    out of range or of the wrong kind (raised before any library call)."""

    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("lightsheet: {} must be a number, not {!r}".format(name, v))
        return v

    p = float(number("percentile", percentile))
    if not (0.0 < p < 1.0):  # (nan fails both comparisons)
        raise ValueError("lightsheet: percentile must lie in (0, 1), not {!r}".format(percentile))
    sizes = []
    for name, v, top in (("artifact_length", artifact_length, LIGHTSHEET_MAX_ARTIFACT),
                         ("background_window_size", background_window_size, LIGHTSHEET_MAX_WINDOW)):  # fmt: skip
        v = number(name, v)
        if not np.isfinite(v) or int(v) != v or not (1 <= int(v) <= top):
            raise ValueError("lightsheet: {} must be an integer in 1 .. {}, not {!r}".format(name, top, v))
        sizes.append(int(v))
    lam = float(number("lightsheet_vs_background", lightsheet_vs_background))
    if not (lam > 0.0 and np.isfinite(np.float32(lam)) and np.float32(lam) > 0):
        raise ValueError("lightsheet: lightsheet_vs_background must be positive and finite, not {!r}".format(
            lightsheet_vs_background))  # fmt: skip
    return p, sizes[0], sizes[1], lam


def lightsheet_tables():
    """``(edges, back)`` of the light-sheet mode's fixed log scale ``q = floor(255 log2(1 + x) / 16)``, made in NumPy
    float64: ``edges[v - 1]`` (uint32, v = 1 .. 255) the smallest ``x`` with ``q(x) >= v``, and ``back[v] =
    float32(2 ** (16 v / 255) - 1)``.  The plan, the host build and the NumPy restatement of the tests all take them."""
    x = np.arange(65536, dtype=np.float64)
    q = np.floor(255.0 * np.log2(1.0 + x) / 16.0).astype(np.int64)
    edges = np.searchsorted(q, np.arange(1, 256), side="left").astype(np.uint32)
    back = (np.exp2(16.0 * np.arange(256, dtype=np.float64) / 255.0) - 1.0).astype(np.float32)
    return edges, back


def lightsheet_ref(plane, percentile=0.25, artifact_length=150, background_window_size=200,
                   lightsheet_vs_background=2.0, out_dtype=np.float32, tables=None):  # fmt: skip
    """Host build of the light-sheet background mode over one uint16 plane (``dsx_lightsheet_ref``): returns ``(out, ls,
    bg)``, ``out`` of ``out_dtype`` (uint16 / float32) and the two uint8 percentile planes.  No GPU involved."""
    p, A, B, lam = lightsheet_params(percentile, artifact_length, background_window_size, lightsheet_vs_background)
    a = np.ascontiguousarray(plane)
    if a.ndim != 2 or a.dtype != np.uint16 or a.size == 0:
        raise ValueError("lightsheet: the plane must be a non-empty 2-D uint16 array")
    edges, back = lightsheet_tables() if tables is None else tables
    edges, back = np.ascontiguousarray(edges, np.uint32), np.ascontiguousarray(back, np.float32)
    if edges.shape != (255,) or back.shape != (256,):
        raise ValueError("lightsheet: tables must be (255 uint32 edges, 256 float32 values)")
    out = np.empty(a.shape, np.dtype(out_dtype))
    ls, bg = np.empty(a.shape, np.uint8), np.empty(a.shape, np.uint8)
    lib = load_library()
    rc = lib.dsx_lightsheet_ref(a.ctypes.data, a.shape[0], a.shape[1], p, A, B, lam, edges.ctypes.data, back.ctypes.data,
                                ls.ctypes.data, bg.ctypes.data, out.ctypes.data, _dtype_code(out.dtype))  # fmt: skip
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"lightsheet_ref failed").decode())
    return out, ls, bg


def rot90_ref(planes, direction=1):
    """``np.rot90`` (``direction=1``) or ``np.rot90(., -1)`` (``-1``) of every plane of ``planes[n, H, W]`` (uint16 /
    float32) through ``dsx_rot90_ref``: the host build of the index map ``k_rot90`` uses.  No GPU involved."""
    a = np.ascontiguousarray(planes)
    if a.ndim != 3:
        raise ValueError("planes must be [n, H, W]")
    n, H, W = a.shape
    out = np.empty((n, W, H), a.dtype)
    rc = load_library().dsx_rot90_ref(a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                      _dtype_code(a.dtype), n, H, W, int(direction))  # fmt: skip
    if rc != 0:
        raise ValueError(load_library().dsx_last_error(None).decode())
    return out


def _shading_planes(flatfield, darkfield, out_shape):
    """float32 flat / dark of a plan, with the checks (and messages) of ``flatfield_correction()``,
    filtering.py:377-391: the dark is at least the plane (cropped by indexing), the flat is the plane."""
    flat = np.ascontiguousarray(flatfield, dtype=np.float32)
    dark = np.ascontiguousarray(darkfield, dtype=np.float32)
    if flat.ndim != 2 or dark.ndim != 2:
        raise ValueError("flatfield / darkfield must be 2-D planes")
    cropped = dark[: out_shape[0], : out_shape[1]].shape
    if cropped != out_shape:
        raise ValueError(
            "Please, check the shape of the darkfield. "
            "Image: {} - Darkfield: {}".format(out_shape, cropped)
        )
    if flat.shape != out_shape:
        raise ValueError(
            "Please, check the shape of the flatfield."
            "Image: {} - Flatfield: {}".format(out_shape, flat.shape)
        )
    return flat, dark
# What "auto" resolves to where the march route applies.  The march route's rate has not been measured, so "auto" is the
# generic route everywhere; it becomes "march" here once a same-session record (tools/bench_streaks.py with both
# routes, README "filter_streaks") shows march ahead.  Elsewhere "auto" is the generic route in any case.
AUTO_ROUTE = "generic"


def _db3_max_level(height, width):
    def one(n):  # pywt.dwt_max_level(n, 6)
        return 0 if n < 5 else max(0, int(math.floor(math.log2(n // 5))))

    return min(one(int(height)), one(int(width)))


def streaks_route(route, height, width, wavelet="db3", level=0):
    """The route a streaks plan takes: ``"auto"`` resolved, ``ValueError`` for a name that is none of ``generic`` /
    ``march`` / ``auto`` and for ``"march"`` where it does not apply (it takes db3, even height and width and a
    ``level`` up to the maximum level)."""
    if route not in ("generic", "march", "auto"):
        raise ValueError("route must be 'generic', 'march' or 'auto', not {!r}".format(route))
    if route == "generic":
        return route
    applies = (_wavelet_key({"wavelet": wavelet}) == "db3" and int(height) % 2 == 0 and int(width) % 2 == 0
               and int(level or 0) <= _db3_max_level(height, width))  # fmt: skip
    if route == "march":
        if not applies:
            raise ValueError("route 'march' takes the db3 wavelet, planes of even height and width and levels up to "
                             "the maximum level only")  # fmt: skip
        return route
    return AUTO_ROUTE if applies else "generic"


def _wavelet_key(cfg):
    w = cfg.get("wavelet", "db3")
    return w.lower() if isinstance(w, str) else w


def _as_cfg(cfg):
    """Reference config dict {"wavelet","level","sigma","max_threshold"} -> C struct."""
    wid = DSX_WAVELET_DB3 if _wavelet_key(cfg) == "db3" and not os.environ.get("DSX_GENERIC_DB3") else DSX_WAVELET_BANK
    level = cfg.get("level", 0)
    return _Cfg(wid, -1 if level is None else int(level), float(cfg.get("sigma", 64)),
                float(cfg.get("max_threshold", 4)))  # fmt: skip


class DeviceBuffer:
    """A device allocation owned by an engine."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        engine._check(engine._lib.dsx_malloc(engine._ctx, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr is not None and self.engine._ctx is not None:
            self.engine._lib.dsx_free(self.engine._ctx, ctypes.c_void_p(self.ptr))
        self.ptr = None

    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array)
        assert offset + a.nbytes <= self.nbytes
        self.engine._check(
            self.engine._lib.dsx_memcpy_h2d(self.engine._ctx, ctypes.c_void_p(self.ptr + offset),
                                            a.ctypes.data_as(ctypes.c_void_p), a.nbytes)
        )  # fmt: skip

    def download(self, shape, dtype, offset=0):
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        self.engine._check(
            self.engine._lib.dsx_memcpy_d2h(self.engine._ctx, out.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.c_void_p(self.ptr + offset), out.nbytes)
        )  # fmt: skip
        return out


class PinnedBuffer:
    """Page-locked host memory owned by an engine (``dsx_malloc_host``): async copies need it."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        engine._check(engine._lib.dsx_malloc_host(engine._ctx, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def array(self, shape, dtype, offset=0):
        """NumPy view of (part of) the buffer."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert offset + n <= self.nbytes
        raw = (ctypes.c_char * n).from_address(self.ptr + offset)
        return np.frombuffer(raw, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr is not None and self.engine._ctx is not None:
            self.engine._lib.dsx_free_host(self.engine._ctx, ctypes.c_void_p(self.ptr))
        self.ptr = None


def _dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return DSX_U16
    if dtype == np.float32:
        return DSX_F32
    raise ValueError("planes must be uint16 or float32, got {}".format(dtype))


class DestripeEngine:
    """One context on one GPU: ``plan()`` once per plane geometry / config pair, then ``run()``."""

    def __init__(self, device=0):
        self._lib = load_library()
        ctx = ctypes.c_void_p()
        rc = self._lib.dsx_init(int(device), ctypes.byref(ctx))
        if rc != 0:
            msg = self._lib.dsx_last_error(None)
            raise DsxError(rc, msg.decode() if msg else "dsx_init failed")
        self._ctx = ctx
        self.device = int(device)
        self.info = None
        self.streaks_route = None  # route of the current plan when it is a streaks plan

    # -- plumbing --------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            msg = self._lib.dsx_last_error(self._ctx)
            if rc == -8:  # DSX_EVALUE: the reference's own exception type and message (numpy.histogram)
                raise ValueError(msg.decode() if msg else "autodetected range of [nan, nan] is not finite")
            raise DsxError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_ctx", None) is not None:
            self._lib.dsx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plan ------------------------------------------------------------------------------------
    def plan(self, height, width, cells_config, no_cells_config, microscope_high_int=2700,
             max_batch=32, flatfield=None, darkfield=None, rotate=False):  # fmt: skip
        """``rotate=True`` (``dsx_set_rotate``): the plan computes ``np.rot90(F(np.rot90(x)), -1)`` per plane, ``F``
        the plan without it -- vertical stripes.  ``height`` / ``width``, the planes of :meth:`run`, ``flatfield`` and
        ``darkfield`` stay in the caller's orientation; ``info.level_h`` / ``level_w`` are the rotated chain's."""
        rotate = rotate_flag(rotate)
        cells, no_cells = _as_cfg(cells_config), _as_cfg(no_cells_config)
        # Both configs go through ONE decomposition: which config a plane takes is only known once the
        # statistic fused into the level-1 analysis is (filtering.py:455-462 decides before it transforms).
        if _wavelet_key(cells_config) != _wavelet_key(no_cells_config):
            raise ValueError("cells_config and no_cells_config must name the same wavelet")
        if cells.wavelet == DSX_WAVELET_BANK:  # anything but db3: hand the filter bank over (DSX_GENERIC_DB3: db3 too)
            bank = [np.ascontiguousarray(f, dtype=np.float64) for f in wavelets.filter_bank(_wavelet_key(cells_config))]
            dp = ctypes.POINTER(ctypes.c_double)
            rc = self._lib.dsx_set_wavelet(self._ctx, *[f.ctypes.data_as(dp) for f in bank], len(bank[0]))
            if rc == -1:
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)

        self._check(self._lib.dsx_set_rotate(self._ctx, 1 if rotate else 0))

        def call(flat_p, dark_p, dark_h, dark_w):
            rc = self._lib.dsx_plan(self._ctx, int(height), int(width), int(max_batch), ctypes.byref(cells),
                                    ctypes.byref(no_cells), float(microscope_high_int), flat_p, dark_p,
                                    int(dark_h), int(dark_w))  # fmt: skip
            if rc == -1:  # the reference raises ValueError for these (filtering.py:107-112, 379-391)
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)
            info = _PlanInfo()
            self._check(self._lib.dsx_plan_info(self._ctx, ctypes.byref(info)))
            return info

        if (flatfield is None) != (darkfield is None):
            raise ValueError("flatfield and darkfield must be given together")
        info = call(None, None, 0, 0)
        if flatfield is not None:
            flat, dark = _shading_planes(flatfield, darkfield, (info.out_height, info.out_width))
            info = call(flat.ctypes.data_as(ctypes.c_void_p), dark.ctypes.data_as(ctypes.c_void_p),
                        dark.shape[0], dark.shape[1])  # fmt: skip
        self.info = info
        self.streaks_route = None
        return info

    def plan_streaks(self, height, width, sigma_fg, sigma_bg, wavelet="db3", level=0, crossover=10.0,
                     threshold=None, max_batch=32, route="generic", bands="both", smoothing=0.0, flatfield=None,
                     darkfield=None, rotate=False):  # fmt: skip
        """Plan the dual-band filter (``dsx_plan_streaks_ex``); ``threshold=None``: Otsu per plane.  Replaces any plan
        of this engine; :meth:`run` / :meth:`run_device` then return ``[n, height, width]``.  ``route``: ``"generic"``
        (the per-band kernels of the filter, any wavelet and plane), ``"march"`` (the bands run through the log-space
        db3 chain; db3, even planes and levels up to the maximum only, ``ValueError`` elsewhere) or ``"auto"``
        (``AUTO_ROUTE`` where march applies -- generic until a measurement shows march ahead -- generic elsewhere).

        Options of the blend (``dsx_plan_streaks_opts``; with none given the plan is ``dsx_plan_streaks_ex``):
        ``bands`` ``"both"``, ``"fg"`` (only the foreground band is filtered and blended with the raw plane,
        ``sigma_bg`` is not read) or ``"bg"`` (the same for the background band); ``smoothing`` 0 or ``0 < s <= 2``, the
        sigma of ``scipy.ndimage.gaussian_filter`` over the blend weight; ``flatfield`` / ``darkfield`` (together, shapes
        as in :meth:`plan`): the reference's ``flatfield_correction`` of the blend result.  ``rotate``: as in
        :meth:`plan` (the route conditions are symmetric in height and width)."""
        rotate = rotate_flag(rotate)
        if bands not in STREAKS_BANDS:
            raise ValueError("bands must be 'both', 'fg' or 'bg', not {!r}".format(bands))
        smoothing = streaks_smoothing(smoothing)
        if (flatfield is None) != (darkfield is None):
            raise ValueError("flatfield and darkfield must be given together")
        flat = dark = None
        if flatfield is not None:
            flat, dark = _shading_planes(flatfield, darkfield, (int(height), int(width)))
        if bands == "fg":
            sigma_bg = sigma_fg
        elif bands == "bg":
            sigma_fg = sigma_bg
        route = streaks_route(route, height, width, wavelet, level)
        key = _wavelet_key({"wavelet": wavelet})
        wid = DSX_WAVELET_DB3 if key == "db3" else DSX_WAVELET_BANK
        if wid == DSX_WAVELET_BANK:
            bank = [np.ascontiguousarray(f, dtype=np.float64) for f in wavelets.filter_bank(key)]
            dp = ctypes.POINTER(ctypes.c_double)
            rc = self._lib.dsx_set_wavelet(self._ctx, *[f.ctypes.data_as(dp) for f in bank], len(bank[0]))
            if rc == -1:
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)
        cfg = _StreaksCfg(wid, int(level or 0), float(sigma_fg), float(sigma_bg), float(crossover),
                          1 if threshold is None else 0, 0.0 if threshold is None else float(threshold))  # fmt: skip
        opts = _StreaksOpts(STREAKS_BANDS[bands], smoothing, None if flat is None else flat.ctypes.data,
                            None if dark is None else dark.ctypes.data, 0 if dark is None else dark.shape[0],
                            0 if dark is None else dark.shape[1])  # fmt: skip
        self._check(self._lib.dsx_set_rotate(self._ctx, 1 if rotate else 0))
        rc = self._lib.dsx_plan_streaks_opts(self._ctx, int(height), int(width), int(max_batch), ctypes.byref(cfg),
                                             STREAKS_ROUTES[route], ctypes.byref(opts))  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)
        info = _PlanInfo()
        info.height, info.width, info.out_height, info.out_width = int(height), int(width), int(height), int(width)
        info.max_batch = int(max_batch)
        self.info = info
        self.streaks_route = route
        return info

    def plan_lightsheet(self, height, width, percentile=0.25, artifact_length=150, background_window_size=200,
                        lightsheet_vs_background=2.0, max_batch=32, rotate=False, tables=None):  # fmt: skip
        """Plan the light-sheet background mode (``dsx_plan_lightsheet``).  Replaces any plan of this engine;
        :meth:`run` / :meth:`run_device` then take uint16 planes and return ``[n, height, width]`` uint16 or float32.
        ``rotate``: as in :meth:`plan`.  ``tables``: ``(edges, back)``, by default :func:`lightsheet_tables`."""
        rotate = rotate_flag(rotate)
        p, A, B, lam = lightsheet_params(percentile, artifact_length, background_window_size, lightsheet_vs_background)
        edges, back = lightsheet_tables() if tables is None else tables
        edges, back = np.ascontiguousarray(edges, np.uint32), np.ascontiguousarray(back, np.float32)
        if edges.shape != (255,) or back.shape != (256,):
            raise ValueError("lightsheet: tables must be (255 uint32 edges, 256 float32 values)")
        self._check(self._lib.dsx_set_rotate(self._ctx, 1 if rotate else 0))
        rc = self._lib.dsx_plan_lightsheet(self._ctx, int(height), int(width), int(max_batch), p, A, B, lam,
                                           edges.ctypes.data, back.ctypes.data)  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)
        info = _PlanInfo()
        info.height, info.width, info.out_height, info.out_width = int(height), int(width), int(height), int(width)
        info.max_batch = int(max_batch)
        self.info = info
        self.streaks_route = None
        self._ls_shape = (int(width), int(height)) if rotate else (int(height), int(width))
        return info

    def lightsheet_planes(self, plane):
        """``(ls, bg)``: the two uint8 percentile planes of a plane of the last cohort of a light-sheet run
        (``dsx_get_lightsheet_planes``), in the plan's own orientation (the rotated one of a ``rotate=True`` plan)."""
        ls, bg = np.empty(self._ls_shape, np.uint8), np.empty(self._ls_shape, np.uint8)
        self._check(self._lib.dsx_get_lightsheet_planes(self._ctx, int(plane), ls.ctypes.data, bg.ctypes.data))
        return ls, bg

    def streaks_threshold(self, plane):
        """Threshold ``t`` of a plane of the last cohort of a streaks run (``dsx_get_streaks_threshold``)."""
        t = ctypes.c_float()
        self._check(self._lib.dsx_get_streaks_threshold(self._ctx, int(plane), ctypes.byref(t)))
        return float(t.value)

    def graph_stats(self):
        """``(graph launches, captures)`` of this context (``dsx_graph_stats``)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.dsx_graph_stats(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def row_pack_launches(self):
        """Launches of the packed coarse row filter this context has enqueued (``dsx_row_pack_launches``)."""
        n = ctypes.c_uint64()
        self._check(self._lib.dsx_row_pack_launches(self._ctx, ctypes.byref(n)))
        return int(n.value)

    @property
    def out_shape(self):
        return (self.info.out_height, self.info.out_width)

    @property
    def levels(self):
        return self.info.levels

    def level_shape(self, level):
        return (self.info.level_h[level], self.info.level_w[level])

    # -- run -------------------------------------------------------------------------------------
    def run(self, planes, out_dtype=np.float32, return_cfg=False):
        """Host arrays in, host arrays out: ``planes[n, H, W]`` (uint16 / float32)."""
        a = np.ascontiguousarray(planes)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.info.height, self.info.width):
            raise ValueError("planes must be [n, {}, {}]".format(self.info.height, self.info.width))
        n = a.shape[0]
        out = np.empty((n,) + self.out_shape, dtype=out_dtype)
        cfg = np.zeros(n, dtype=np.int32)
        self._check(
            self._lib.dsx_run_host(self._ctx, a.ctypes.data_as(ctypes.c_void_p), _dtype_code(a.dtype), n,
                                   out.ctypes.data_as(ctypes.c_void_p), _dtype_code(out.dtype),
                                   cfg.ctypes.data_as(ctypes.c_void_p))
        )  # fmt: skip
        return (out, cfg) if return_cfg else out

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def run_device(self, d_in, in_dtype, n, d_out, out_dtype, d_cfg=None):
        """Device buffers; asynchronous on the engine stream."""
        self._check(
            self._lib.dsx_run_device(self._ctx, ctypes.c_void_p(d_in.ptr), _dtype_code(in_dtype), int(n),
                                     ctypes.c_void_p(d_out.ptr), _dtype_code(out_dtype),
                                     ctypes.c_void_p(d_cfg.ptr) if d_cfg is not None else None)
        )  # fmt: skip

    def sync(self):
        self._check(self._lib.dsx_sync(self._ctx))

    def blosc_encode_device(self, d_src, n_chunks, chunk_bytes, d_frames, d_offsets, typesize=2, clevel=3,
                            mode="literals"):
        """Blosc frames of ``n_chunks`` chunks of ``chunk_bytes`` (device buffer ``d_src``), encoded on the device into
        ``d_frames`` (capacity ``n_chunks * (chunk_bytes + 16)``), packed back to back; ``d_offsets`` receives
        ``n_chunks + 1`` int64 frame offsets.  ``mode``, one of :data:`ZENC_MODES`: ``"literals"`` = Blosc-zstd frames,
        entropy coding only; ``"runs"`` = Blosc-zstd frames in which runs of equal bytes become matches; ``"lz4"`` =
        Blosc-LZ4 frames with split streams (``csrc/dsx_lz4_enc.h``).  Asynchronous on the engine stream."""
        self._check(self._lib.dsx_blosc_encode_device_ex(self._ctx, ctypes.c_void_p(d_src.ptr), int(n_chunks),
                                                         int(chunk_bytes), int(typesize), int(clevel),
                                                         ctypes.c_void_p(d_frames.ptr), ctypes.c_void_p(d_offsets.ptr),
                                                         zenc_mode(mode)))  # fmt: skip

    def timer_start(self):
        self._check(self._lib.dsx_timer_start(self._ctx))

    def timer_stop(self):
        ms = ctypes.c_float()
        self._check(self._lib.dsx_timer_stop(self._ctx, ctypes.byref(ms)))
        return ms.value

    def constants_device(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._lib.dsx_constants_device(self._ctx, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # -- multi-GPU: RCCL communicator (include/dsx.h, dsx_comm_*) --------------------------------
    def comm_unique_id(self):
        """128-byte RCCL unique id; rank 0 creates it and hands it to the other ranks (any host channel)."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        self._check(self._lib.dsx_comm_unique_id(self._ctx, buf, COMM_ID_BYTES))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """Collective over all ranks of the job."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("the RCCL unique id has {} bytes".format(COMM_ID_BYTES))
        self._check(self._lib.dsx_comm_init(self._ctx, bytes(unique_id), COMM_ID_BYTES, int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._lib.dsx_comm_destroy(self._ctx))

    def comm_broadcast(self, d_ptr, nbytes, root=0):
        """In-place RCCL broadcast of device memory (address or DeviceBuffer) from ``root``."""
        ptr = d_ptr.ptr if isinstance(d_ptr, DeviceBuffer) else d_ptr
        self._check(self._lib.dsx_comm_broadcast(self._ctx, ctypes.c_void_p(ptr), int(nbytes), int(root)))

    def blosc_decode_device(self, d_packed, packed_bytes, d_tasks, n_tasks, d_out, d_status, out_bytes=None):
        """The tasks of :meth:`io_read_frames` (device buffers: packed frames, ``TASK_DTYPE`` table) decoded into
        ``d_out``; ``d_status`` receives one int32 per task (0 = exact output).  Asynchronous on the engine stream."""
        self._check(self._lib.dsx_blosc_decode_device(self._ctx, ctypes.c_void_p(d_packed.ptr), int(packed_bytes),
                                                      ctypes.c_void_p(d_tasks.ptr), int(n_tasks),
                                                      ctypes.c_void_p(d_out.ptr),
                                                      int(d_out.nbytes if out_bytes is None else out_bytes),
                                                      ctypes.c_void_p(d_status.ptr)))  # fmt: skip

    def comm_allreduce(self, values, op="sum"):
        """All-reduce of a few host doubles over the ranks (also a barrier): op sum / max / min."""
        v = (ctypes.c_double * len(values))(*[float(x) for x in values])
        self._check(self._lib.dsx_comm_allreduce_f64(self._ctx, v, len(values), {"sum": 0, "max": 1, "min": 2}[op]))
        return [float(x) for x in v]

    # -- pinned staging + copy streams (overlapped chunk map) ------------------------------------
    def alloc_host(self, nbytes):
        return PinnedBuffer(self, nbytes)

    def copy_h2d_async(self, d_buf, host_array, stream=STREAM_UPLOAD, offset=0):
        a = host_array
        assert a.flags["C_CONTIGUOUS"] and offset + a.nbytes <= d_buf.nbytes
        self._check(self._lib.dsx_memcpy_h2d_async(self._ctx, ctypes.c_void_p(d_buf.ptr + offset),
                                                   a.ctypes.data_as(ctypes.c_void_p), a.nbytes, int(stream)))  # fmt: skip

    def copy_d2h_async(self, host_array, d_buf, stream=STREAM_DOWNLOAD, offset=0):
        a = host_array
        assert a.flags["C_CONTIGUOUS"] and offset + a.nbytes <= d_buf.nbytes
        self._check(self._lib.dsx_memcpy_d2h_async(self._ctx, a.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.c_void_p(d_buf.ptr + offset), a.nbytes, int(stream)))  # fmt: skip

    def stream_wait(self, waiter, signaller):
        self._check(self._lib.dsx_stream_wait(self._ctx, int(waiter), int(signaller)))

    def stream_sync(self, stream):
        self._check(self._lib.dsx_stream_sync(self._ctx, int(stream)))

    # -- chunk files on native threads (dsx_io.h); ctypes releases the GIL for the call -----------
    def io_read_chunks(self, paths, arrays, threads=16, zlib_chunks=False, fill_value=0, codec=None):
        """Chunk files ``paths[i]`` -> ``arrays[i]`` (C-contiguous NumPy arrays of the decompressed chunk size).
        ``codec``: ``DSX_CODEC_*`` (0 raw, 1 zlib, 2 Blosc); default from ``zlib_chunks``."""
        n = len(paths)
        cp = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
        dp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])
        nb = (ctypes.c_size_t * n)(*[a.nbytes for a in arrays])
        code = (1 if zlib_chunks else 0) if codec is None else int(codec)
        self._check(self._lib.dsx_io_read_chunks(self._ctx, cp, dp, nb, n, int(threads), code, int(fill_value)))

    def io_write_chunks(self, paths, arrays, threads=16, zlib_level=-1, blosc=None):
        """``arrays[i]`` -> chunk files ``paths[i]`` (raw, zlib streams for ``zlib_level >= 0``, Blosc-zstd frames for
        ``blosc = (clevel, typesize, shuffle)``, or Blosc-LZ4 frames of uint16 for ``blosc = (clevel, 2, True, "lz4")``:
        what ``MiniZarrArray.blosc_write_params`` returns), atomically."""
        n = len(paths)
        cp = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
        dp = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])
        nb = (ctypes.c_size_t * n)(*[a.nbytes for a in arrays])
        if blosc is not None and len(blosc) == 4:
            clevel, typesize, shuffle, cname = blosc
            if cname != "lz4" or typesize != 2 or not shuffle:
                raise ValueError("Blosc-LZ4 chunks are written byte-shuffled at typesize 2, not {!r}".format(blosc))
            self._check(self._lib.dsx_io_write_chunks_blosc_lz4(self._ctx, cp, dp, nb, n, int(threads), int(clevel)))
            return
        if blosc is not None:
            clevel, typesize, shuffle = blosc
            self._check(self._lib.dsx_io_write_chunks_blosc(self._ctx, cp, dp, nb, n, int(threads), int(clevel),
                                                            int(typesize), 1 if shuffle else 0))  # fmt: skip
            return
        self._check(self._lib.dsx_io_write_chunks(self._ctx, cp, dp, nb, n, int(threads), int(zlib_level)))

    def io_read_frames(self, paths, chunk_bytes, packed, tasks, threads=16, fill_value=0, routes=None, mode=0,
                       zlib_chunks=False):
        """Chunk files ``paths[i]`` (Blosc) -> frames packed into the uint8 array ``packed`` and Blosc block tasks
        into the ``TASK_DTYPE`` array ``tasks`` (``dsx_io_read_frames``); chunk i decodes to bytes
        ``[i * chunk_bytes, (i + 1) * chunk_bytes)``.  ``routes``: optional uint8 array of ``len(paths)`` (``ROUTE_*``).
        ``mode``: ``ZDEC_ZSTD`` (0: unsplit zstd streams go to the device) or ``ZDEC_ANY`` (1: LZ4, split streams and
        bit shuffle too, ``dsx_io_read_frames_ex``) or ``ZDEC_ALL`` (3: blosclz and zlib inside too).
        ``zlib_chunks``: the files are the chunks of a plain-zlib store, one ``TASK_ZLIB`` task each
        (``dsx_io_read_zlib_chunks``; ``mode`` does not apply).  Returns ``(packed_bytes, n_tasks)``."""
        return _io_read_frames(self._lib, self._ctx, paths, chunk_bytes, packed, tasks, threads, fill_value, routes,
                               self._check, mode, zlib_chunks)  # fmt: skip

    def event_record(self, slot, stream):
        self._check(self._lib.dsx_event_record(self._ctx, int(slot), int(stream)))

    def event_sync(self, slot):
        self._check(self._lib.dsx_event_sync(self._ctx, int(slot)))

    def copy_d2d_async(self, d_dst, d_src, nbytes):
        self._check(self._lib.dsx_memcpy_d2d(self._ctx, ctypes.c_void_p(d_dst.ptr), ctypes.c_void_p(d_src.ptr), int(nbytes)))

    def profile(self, on):
        self._check(self._lib.dsx_profile_enable(self._ctx, 1 if on else 0))

    def profile_read(self):
        ms = (ctypes.c_float * 16)()
        cnt = (ctypes.c_int32 * 16)()
        names = (ctypes.c_char_p * 16)()
        n = ctypes.c_int()
        self._check(self._lib.dsx_profile_read(self._ctx, 16, ms, cnt, names, ctypes.byref(n)))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}

    # -- data formats either side of the filter (device buffers, asynchronous) -------------------
    def bricks_to_planes(self, d_bricks, d_planes, zyx, brick, z0=0):
        """Zarr chunk order -> dense ``[Z, H, W]`` uint16 (``zarr_destriper.py:1066-1074``)."""
        self._check(self._lib.dsx_bricks_to_planes_u16(self._ctx, ctypes.c_void_p(d_bricks.ptr),
                                                       ctypes.c_void_p(d_planes.ptr), *map(int, zyx),
                                                       *map(int, brick), int(z0)))  # fmt: skip

    def planes_to_bricks(self, d_planes, d_bricks, zyx, brick, z0=0):
        """Dense ``[Z, H, W]`` uint16 -> Zarr chunk order, 0 outside the stack (``zarr_destriper.py:336``)."""
        self._check(self._lib.dsx_planes_to_bricks_u16(self._ctx, ctypes.c_void_p(d_planes.ptr),
                                                       ctypes.c_void_p(d_bricks.ptr), *map(int, zyx),
                                                       *map(int, brick), int(z0)))  # fmt: skip

    def downsample2(self, d_src, d_dst, zyx, scale=(2, 2, 2)):
        """One windowed-mean pyramid level, uint16 (``zarr_destriper.py:365-407``): ``zyx`` -> ``zyx // scale``, the
        window ``scale`` = 1 or 2 per axis (``dsx_downsample_u16``; 2 x 2 x 2 is ``dsx_downsample2_u16``)."""
        scale = pyramid_scale(scale)
        assert d_src.nbytes >= int(np.prod(zyx)) * 2, "downsample source buffer too small"
        assert d_dst.nbytes >= int(np.prod([n // f for n, f in zip(zyx, scale)])) * 2, "downsample buffer too small"
        rc = self._lib.dsx_downsample_u16(self._ctx, ctypes.c_void_p(d_src.ptr), ctypes.c_void_p(d_dst.ptr),
                                          *map(int, zyx), *scale)  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)

    def pyramid_block(self, d_planes, zyx, chunks, d_bricks, z0s=None, zero=None, rows=None, d_work=None, scale=(2, 2, 2)):
        """Pyramid levels ``1 .. len(chunks)`` of the dense uint16 block ``d_planes`` (``zyx``), each stored in chunk
        order into ``d_bricks[l - 1]`` (``dsx_pyramid_block_scale_u16``; ``zarr_destriper.py:365-407, 746-782``).

        ``chunks[l - 1]``: the level's (clamped) chunk shape; ``z0s[l - 1]``: first plane of the block's share inside the
        level's brick grid (default 0); ``zero[l - 1]``: zero the level's buffer first (default True); ``rows[l - 1]``:
        chunk rows the buffer holds (default: what the share needs).  ``d_work``: ``pyramid_work_bytes`` bytes when there
        are more than two levels (more than one with a ``scale`` other than 2 x 2 x 2).  ``scale``: the window per axis,
        1 or 2 each.  Asynchronous on the engine stream."""
        scale = pyramid_scale(scale)
        table = _pyramid_table(zyx, chunks, z0s, zero, rows, scale)
        n = len(chunks)
        assert d_planes.nbytes >= int(np.prod(zyx)) * 2, "pyramid source buffer too small"
        assert n < 2 or scale == (2, 2, 2) or (d_work is not None and d_work.nbytes >= pyramid_work_bytes(zyx, n + 1, scale))
        for lv, g, b in zip(range(1, n + 1), table, d_bricks):
            assert b.nbytes >= pyramid_level_elems(zyx, lv, (g.cz, g.cy, g.cx), g.rows, scale) * 2, "pyramid brick buffer too small"
        ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ptr for b in d_bricks])
        rc = self._lib.dsx_pyramid_block_scale_u16(self._ctx, ctypes.c_void_p(d_planes.ptr), *map(int, zyx), *scale, n + 1,
                                                   table, ptrs,
                                                   ctypes.c_void_p(d_work.ptr) if d_work is not None else None,
                                                   d_work.nbytes if d_work is not None else 0)  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)

    def pyramid_bricks(self, d_src, zyx, src_chunk, chunks, d_bricks, z0s=None, zero=None, rows=None, d_work=None,
                       scale=(2, 2, 2)):  # fmt: skip
        """:meth:`pyramid_block` for a block that is still in chunk order (``dsx_pyramid_bricks_scale_u16``;
        ``zarr_destriper.py:365-407, 746-782``): ``d_src`` holds the uint16 bricks ``[nbz, nby, nbx] + src_chunk`` of
        the block ``zyx``, which starts on a source chunk boundary; positions outside ``zyx`` are never read.  Every
        other argument as in :meth:`pyramid_block`.  Asynchronous on the engine stream."""
        scale = pyramid_scale(scale)
        table = _pyramid_table(zyx, chunks, z0s, zero, rows, scale)
        n = len(chunks)
        assert d_src.nbytes >= src_brick_elems(zyx, src_chunk) * 2, "pyramid source brick buffer too small"
        assert n < 2 or scale == (2, 2, 2) or (d_work is not None and d_work.nbytes >= pyramid_work_bytes(zyx, n + 1, scale))
        for lv, g, b in zip(range(1, n + 1), table, d_bricks):
            assert b.nbytes >= pyramid_level_elems(zyx, lv, (g.cz, g.cy, g.cx), g.rows, scale) * 2, "pyramid brick buffer too small"
        ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ptr for b in d_bricks])
        rc = self._lib.dsx_pyramid_bricks_scale_u16(self._ctx, ctypes.c_void_p(d_src.ptr), *map(int, zyx),
                                                    *map(int, src_chunk), *scale, n + 1, table, ptrs,
                                                    ctypes.c_void_p(d_work.ptr) if d_work is not None else None,
                                                    d_work.nbytes if d_work is not None else 0)  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)

    # -- histogram of the written volume (display window of the OME-NGFF metadata) ---------------
    def volhist_reset(self):
        """Zero the engine's 65 536-bin voxel histogram (``dsx_volhist_reset``; allocated on first use)."""
        self._check(self._lib.dsx_volhist_reset(self._ctx))

    def volhist_add(self, d_buf_or_ptr, n):
        """Count ``n`` contiguous uint16 voxels at a :class:`DeviceBuffer` or a device address into the histogram
        (``dsx_volhist_add_device``; ``zarr_destriper.py:722-726``).  Asynchronous on the engine stream."""
        ptr = getattr(d_buf_or_ptr, "ptr", d_buf_or_ptr)
        nbytes = getattr(d_buf_or_ptr, "nbytes", None)
        assert nbytes is None or 2 * int(n) <= nbytes, "volhist_add: more voxels than the buffer holds"
        self._check(self._lib.dsx_volhist_add_device(self._ctx, ctypes.c_void_p(ptr), int(n)))

    def volhist_get(self):
        """The counts so far as ``np.int64[65536]`` (``dsx_volhist_get``; waits for the engine stream)."""
        out = np.zeros(VOLHIST_BINS, np.uint64)
        self._check(self._lib.dsx_volhist_get(self._ctx, out.ctypes.data_as(ctypes.c_void_p)))
        return out.astype(np.int64)

    # -- per-pixel order statistics of a plane stack (the samples of flatfield_estimation.py) ------
    def stack_rank(self, d_planes, n, plane_elems, q_milli, valid_range=(0, 65535), d_out=None, d_valid=None):
        """Per-pixel quantiles of ``n`` dense uint16 planes of ``plane_elems`` elements at a :class:`DeviceBuffer` or a
        device address (``dsx_stack_rank_u16_device``; ``flatfield_estimation.py:43-50``), one read of the stack.  Per
        pixel only the values inside ``valid_range = (lo, hi)`` count, ``m`` of them; quantile ``q`` of ``q_milli``
        (per-mille, up to 4) is the ``(q * (m - 1)) // 1000``-th smallest of them, 0 where ``m == 0``.  Results go to
        ``d_out`` (uint16 ``[len(q_milli), plane_elems]``) and ``d_valid`` (uint16 ``[plane_elems]``, the counts
        ``m``); buffers that are not given are allocated, and the caller frees them.  Returns ``(d_out, d_valid)``.  A
        value outside the limits is a ``ValueError`` before any launch.  Asynchronous on the engine stream."""
        n, plane_elems, q, lo, hi = stack_rank_args(n, plane_elems, q_milli, valid_range)
        ptr = getattr(d_planes, "ptr", d_planes)
        nbytes = getattr(d_planes, "nbytes", None)
        assert nbytes is None or 2 * n * plane_elems <= nbytes, "stack_rank: more planes than the buffer holds"
        if d_out is None:
            d_out = self.alloc(max(2 * len(q) * plane_elems, 16))
        if d_valid is None:
            d_valid = self.alloc(max(2 * plane_elems, 16))
        for buf, need in ((d_out, 2 * len(q) * plane_elems), (d_valid, 2 * plane_elems)):
            held = getattr(buf, "nbytes", None)
            assert held is None or need <= held, "stack_rank: a result buffer is too small"
        rc = self._lib.dsx_stack_rank_u16_device(self._ctx, ctypes.c_void_p(ptr), n, plane_elems, lo, hi,
                                                 (ctypes.c_int * len(q))(*q), len(q),
                                                 ctypes.c_void_p(getattr(d_out, "ptr", d_out)),
                                                 ctypes.c_void_p(getattr(d_valid, "ptr", d_valid)))  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)
        return d_out, d_valid

    # -- the finish of a retrospective flat: fill, Gaussian, mean (csrc/dsx_smooth.h) ---------------
    def gauss_smooth(self, d_in, shape, taps, d_tmp=None, d_out=None, radius=None):
        """The two Gaussian passes of the native finish on a float64 plane ``shape = (H, W)`` at a
        :class:`DeviceBuffer` or a device address (``dsx_gauss_smooth_f64_device``; ``flatfield_estimation.py:15-52``):
        axis 0, then axis 1, ``acc = t_0 a[i]; acc = fma(t_k, a[m(i - k)] + a[m(i + k)], acc)`` with the symmetric fold
        ``m``.  ``taps``: :func:`gauss_taps` or any ``t_0 .. t_r``, ``r <= 256`` (a ``radius`` that is given must be that ``r``).  ``d_out`` may be ``d_in``; ``d_tmp``
        is a third plane.  Buffers that are not given are allocated and the caller frees them.  Returns
        ``(d_out, d_tmp)``.  ``ValueError`` before any launch for arguments outside the limits.  Asynchronous on the
        engine stream."""
        H, W, t = smooth_args(shape, taps, radius)
        need = 8 * H * W
        if d_tmp is None:
            d_tmp = self.alloc(max(need, 16))
        if d_out is None:
            d_out = self.alloc(max(need, 16))
        for buf in (d_in, d_tmp, d_out):
            held = getattr(buf, "nbytes", None)
            assert held is None or need <= held, "gauss_smooth: a buffer is too small"
        rc = self._lib.dsx_gauss_smooth_f64_device(self._ctx, ctypes.c_void_p(getattr(d_in, "ptr", d_in)), H, W,
                                                   t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(t) - 1,
                                                   ctypes.c_void_p(getattr(d_tmp, "ptr", d_tmp)),
                                                   ctypes.c_void_p(getattr(d_out, "ptr", d_out)))  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)
        return d_out, d_tmp

    def flat_finish(self, d_rank, d_valid, stored_shape, shape, n_q, taps, floor, d_flat=None, d_dark=None, d_work=None,
                    radius=None):
        """The native finish of a flat on the device (``dsx_flat_finish_device``; ``flatfield_estimation.py:15-52``):
        from the rank planes ``d_rank`` (uint16 ``[n_q, Hs, Ws]``: flat, then dark) and ``d_valid`` (uint16
        ``[Hs, Ws]``) of :meth:`stack_rank`, over the top-left ``shape = (H, W)`` of ``stored_shape = (Hs, Ws)``: the
        unseen pixels take the median of the seen ones, the plane is smoothed as :meth:`gauss_smooth` does,
        ``flat = float32(max(S / mean, floor))`` with the mean summed in 4096 strided lanes, ``dark = float32(S_dark)``.
        Results go to ``d_flat`` / ``d_dark`` (float32 ``[H, W]``); buffers that are not given are allocated (the work
        buffer is freed here, the results are the caller's).  Returns ``(d_flat, d_dark)``, ``d_dark`` ``None`` when
        ``n_q == 1``.  :class:`NoSeenPixel` (a ``ValueError``) when ``valid`` is 0 all over the image; ``ValueError``
        before any launch for arguments outside the limits.  Returns after the chain has run."""
        Hs, Ws, H, W, n_q, t, floor = flat_finish_args(stored_shape, shape, n_q, taps, floor, radius)
        for buf, need in ((d_rank, 2 * n_q * Hs * Ws), (d_valid, 2 * Hs * Ws)):
            held = getattr(buf, "nbytes", None)
            assert held is None or need <= held, "flat_finish: the rank planes do not fit their buffer"
        own_work = d_work is None
        if own_work:
            d_work = self.alloc(flat_finish_work_bytes((H, W)))
        try:
            if d_flat is None:
                d_flat = self.alloc(max(4 * H * W, 16))
            if d_dark is None and n_q == 2:
                d_dark = self.alloc(max(4 * H * W, 16))
            rc = self._lib.dsx_flat_finish_device(self._ctx, ctypes.c_void_p(getattr(d_rank, "ptr", d_rank)),
                                                  ctypes.c_void_p(getattr(d_valid, "ptr", d_valid)), Hs, Ws, H, W, n_q,
                                                  t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(t) - 1, floor,
                                                  ctypes.c_void_p(getattr(d_flat, "ptr", d_flat)),
                                                  ctypes.c_void_p(getattr(d_dark, "ptr", d_dark)) if n_q == 2 else None,
                                                  ctypes.c_void_p(getattr(d_work, "ptr", d_work)))  # fmt: skip
        finally:
            if own_work:
                d_work.free()
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        if rc == -8:
            raise NoSeenPixel(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)
        return d_flat, (d_dark if n_q == 2 else None)

    # -- QC projections of the volume a pass reads and writes --------------------------------------
    def alloc_projection(self, zyx):
        """Six zeroed device arrays for the projections of a ``zyx`` volume: ``{name: DeviceBuffer}`` for
        :meth:`project` (``PROJECTION_ARRAYS``); the caller frees them."""
        bufs = {}
        for name, shape, dtype in projection_shapes(zyx):
            bufs[name] = self.alloc(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 16))
            bufs[name].upload(np.zeros(shape, dtype))
        return bufs

    def project(self, d_planes, zyx, bufs, z_off=0, first=True, d_work=None):
        """Maximum and sum projections of the ``zyx[0]`` dense uint16 planes ``[H, W]`` at a :class:`DeviceBuffer` or a
        device address, one read of them (``dsx_project_u16_device``): rows ``z_off .. z_off + Z - 1`` of the device
        arrays ``max_y`` / ``sum_y`` ``[., W]`` and ``max_x`` / ``sum_x`` ``[., H]`` of ``bufs`` are written; ``max_z`` /
        ``sum_z`` ``[H, W]`` are overwritten when ``first`` and combined otherwise.  ``d_work``:
        :func:`project_work_bytes` bytes, reusable by the next call; without one the call allocates its own and waits.
        More than 65 536 rows, columns or planes is a ``ValueError`` before any launch.  Asynchronous on the engine
        stream."""
        Z, H, W = _project_geometry(zyx)
        z_off = int(z_off)
        if z_off < 0:
            raise ValueError("project: z_off must not be negative")
        ptr = getattr(d_planes, "ptr", d_planes)
        nbytes = getattr(d_planes, "nbytes", None)
        assert nbytes is None or 2 * Z * H * W <= nbytes, "project: more voxels than the buffer holds"
        for name, shape, dtype in projection_shapes((z_off + Z, H, W)):
            assert bufs[name].nbytes >= int(np.prod(shape)) * np.dtype(dtype).itemsize, "project: {} is too small".format(name)
        if Z == 0:
            return
        need = project_work_bytes((Z, H, W))
        own = self.alloc(need) if d_work is None else None
        work = own if d_work is None else d_work
        assert work.nbytes >= need, "project: the work buffer is smaller than project_work_bytes"
        table = _Projection(*[bufs[name].ptr for name, _, _ in PROJECTION_ARRAYS])
        try:
            rc = self._lib.dsx_project_u16_device(self._ctx, ctypes.c_void_p(ptr), Z, H, W, ctypes.byref(table), z_off,
                                                  1 if first else 0, ctypes.c_void_p(work.ptr))  # fmt: skip
            if rc in (-1, -5):
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)
            if own is not None:
                self.sync()
        finally:
            if own is not None:
                own.free()

    def projection_get(self, bufs, zyx):
        """The six arrays of ``bufs`` (``zyx``: the volume they were allocated for) on the host, ``{name: array}``;
        waits for the engine stream."""
        self.sync()
        return {name: bufs[name].download(shape, dtype) for name, shape, dtype in projection_shapes(zyx)}

    # -- per-chunk content digests of bricks in chunk order (the manifest of a store pass) -------
    def brick_digest(self, d_bricks, grid, chunks, valid, d_out, stream=STREAM_COMPUTE, offset=0):
        """Records of the ``grid = (n0, n1, n2)`` bricks of ``chunks = (c0, c1, c2)`` uint16 voxels that lie back to back
        at a :class:`DeviceBuffer` or a device address (``dsx_brick_digest_u16_device``; ``csrc/dsx_digest.h``);
        ``valid = (v0, v1, v2)`` are the voxels the buffer covers from its chunk-aligned origin.  ``d_out`` receives
        ``prod(grid)`` records of :data:`DIGEST_DTYPE`, from byte ``offset`` on.  What the kernel does not take is a
        ``ValueError`` before any launch.  Asynchronous on ``stream``; never waits."""
        n, c, v = digest_geometry(grid, chunks, valid)
        ptr = getattr(d_bricks, "ptr", d_bricks)
        nbytes = getattr(d_bricks, "nbytes", None)
        bricks = n[0] * n[1] * n[2]
        if nbytes is not None and 2 * bricks * c[0] * c[1] * c[2] > nbytes:
            raise ValueError("brick_digest: {} bricks of {} voxels do not fit a buffer of {} bytes".format(bricks, c, nbytes))
        offset = int(offset)
        if offset < 0 or offset % 8 or offset + bricks * DIGEST_DTYPE.itemsize > d_out.nbytes:
            raise ValueError("brick_digest: {} records at byte {} do not fit d_out ({} bytes; the offset a multiple of 8)"
                             .format(bricks, offset, d_out.nbytes))  # fmt: skip
        rc = self._lib.dsx_brick_digest_u16_device(self._ctx, ctypes.c_void_p(ptr), *n, *c, *v,
                                                   ctypes.c_void_p(d_out.ptr + offset), int(stream))  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)

    def foreground_background(self, image, cutoff, want_mask=True):
        """``(fore_mean, back_mean, mask uint8)`` of a host image (uint16 / float32, any shape)."""
        a = np.ascontiguousarray(image)
        d_img = self.alloc(max(a.nbytes, 16))
        d_mask = self.alloc(max(a.size, 16)) if want_mask else None
        try:
            d_img.upload(a)
            f, b = ctypes.c_double(), ctypes.c_double()
            rc = self._lib.dsx_foreground_background(self._ctx, ctypes.c_void_p(d_img.ptr), _dtype_code(a.dtype), a.size,
                                                     float(cutoff), ctypes.byref(f), ctypes.byref(b),
                                                     ctypes.c_void_p(d_mask.ptr) if want_mask else None)  # fmt: skip
            if rc == -1:
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)
            mask = d_mask.download(a.shape, np.uint8) if want_mask else None
            return f.value, b.value, mask
        finally:
            d_img.free()
            if d_mask is not None:
                d_mask.free()

    def flatfield_correction(self, plane, flatfield, darkfield, baseline=0.0):
        """One host plane (uint16 / float32) through ``dsx_flatfield_correction[_rows]``; uint16 result.
        ``baseline``: a scalar, or one value per plane row."""
        a = np.ascontiguousarray(plane)
        flat = np.ascontiguousarray(flatfield, dtype=np.float32)
        dark = np.ascontiguousarray(darkfield, dtype=np.float32)
        H, W = a.shape
        rows = None
        if np.ndim(baseline) > 0:
            rows = np.ascontiguousarray(baseline, dtype=np.float32).ravel()
            if rows.size != H:
                raise ValueError("a per-row baseline needs one value per plane row ({} != {})".format(rows.size, H))
            baseline = 0.0
        bufs = [self.alloc(max(x.nbytes, 16)) for x in (a, flat, dark)] + [self.alloc(max(H * W * 2, 16))]
        if rows is not None:
            bufs.append(self.alloc(max(rows.nbytes, 16)))
        try:
            for b, x in zip(bufs, (a, flat, dark)):
                b.upload(x)
            if rows is not None:
                bufs[4].upload(rows)
            rc = self._lib.dsx_flatfield_correction_rows(self._ctx, ctypes.c_void_p(bufs[0].ptr), _dtype_code(a.dtype), H, W,
                                                         ctypes.c_void_p(bufs[1].ptr), ctypes.c_void_p(bufs[2].ptr),
                                                         dark.shape[0], dark.shape[1], float(baseline),
                                                         ctypes.c_void_p(bufs[4].ptr) if rows is not None else None,
                                                         ctypes.c_void_p(bufs[3].ptr))  # fmt: skip
            if rc == -1:
                raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
            self._check(rc)
            return bufs[3].download((H, W), np.uint16)
        finally:
            for b in bufs:
                b.free()

    def rot90_device(self, d_src, d_dst, dtype, n, height, width, direction=1):
        """``n`` planes ``[height, width]`` of ``d_src`` turned into ``[width, height]`` planes of ``d_dst``
        (``dsx_rot90_device``): ``direction`` 1 is ``np.rot90``, -1 ``np.rot90(., -1)``.  Asynchronous on the engine
        stream."""
        nbytes = int(n) * int(height) * int(width) * np.dtype(dtype).itemsize
        assert nbytes <= d_src.nbytes and nbytes <= d_dst.nbytes, "rot90_device: more planes than a buffer holds"
        rc = self._lib.dsx_rot90_device(self._ctx, ctypes.c_void_p(d_src.ptr), ctypes.c_void_p(d_dst.ptr),
                                        _dtype_code(dtype), int(n), int(height), int(width), int(direction))  # fmt: skip
        if rc == -1:
            raise ValueError(self._lib.dsx_last_error(self._ctx).decode())
        self._check(rc)

    # -- parity hooks ----------------------------------------------------------------------------
    def set_stack_mode(self, on):
        """Planes of one ``run`` call share one Otsu threshold per level (the reference's 3-D input mode)."""
        self._check(self._lib.dsx_set_stack_mode(self._ctx, 1 if on else 0))

    def set_stop_after(self, stage):
        self._check(self._lib.dsx_set_stop_after(self._ctx, int(stage)))

    def stats(self, plane):
        f, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
        self._check(self._lib.dsx_get_stats(self._ctx, int(plane), ctypes.byref(f), ctypes.byref(b), ctypes.byref(c)))
        return f.value, b.value, c.value

    def thresholds(self, plane, level):
        o, t = ctypes.c_float(), ctypes.c_float()
        self._check(self._lib.dsx_get_thresholds(self._ctx, int(plane), int(level), ctypes.byref(o), ctypes.byref(t)))
        return o.value, t.value

    def level_array(self, plane, level, stage=STAGE_DETAIL):
        out = np.empty(self.level_shape(level), dtype=np.float32)
        self._check(self._lib.dsx_get_level(self._ctx, int(plane), int(level), int(stage),
                                            out.ctypes.data_as(ctypes.c_void_p)))  # fmt: skip
        return out


def pyramid_scale(scale):
    """``(fz, fy, fx)`` of a pyramid as ints: each 1 or 2, not all 1 (what the kernels of ``csrc/dsx_pyramid.h`` take);
    ``ValueError`` otherwise."""
    try:
        f = tuple(int(s) for s in scale)
        exact = all(s == v for s, v in zip(scale, f))
    except (TypeError, ValueError):
        f, exact = (), False
    if len(f) != 3 or not exact or any(v not in (1, 2) for v in f) or f == (1, 1, 1):
        raise ValueError("only scale factors of 1 or 2 per axis (not all 1) are implemented, not {!r}".format(scale))
    return f


def pyramid_extent(n, level, factor):
    """Extent of an axis of ``n`` voxels at pyramid level ``level``: halved per level with factor 2, kept with 1."""
    return int(n) >> level if int(factor) == 2 else int(n)


def _pyramid_table(zyx, chunks, z0s, zero, rows, scale=(2, 2, 2)):
    n = len(chunks)
    table = (_PyramidLevel * max(n, 1))()
    for i, ck in enumerate(chunks):
        z0 = int(z0s[i]) if z0s is not None else 0
        share = pyramid_extent(zyx[0], i + 1, scale[0])
        need = max(1, -(-(z0 + share) // int(ck[0])))
        table[i] = _PyramidLevel(int(ck[0]), int(ck[1]), int(ck[2]), int(rows[i]) if rows is not None else need, z0,
                                 1 if zero is None or zero[i] else 0)  # fmt: skip
    return table


def pyramid_level_elems(zyx, level, chunk, rows=1, scale=(2, 2, 2)):
    """uint16 elements of ``rows`` chunk rows of pyramid level ``level`` of a ``[.., H, W]`` volume in chunk order."""
    nby = -(-pyramid_extent(zyx[1], level, scale[1]) // int(chunk[1]))
    nbx = -(-pyramid_extent(zyx[2], level, scale[2]) // int(chunk[2]))
    return int(rows) * nby * nbx * int(chunk[0]) * int(chunk[1]) * int(chunk[2])


def src_brick_elems(zyx, src_chunk):
    """uint16 elements of the block ``zyx`` in the chunk order of an array with chunks ``src_chunk`` (whole bricks)."""
    n = 1
    for e, c in zip(zyx, src_chunk):
        n *= -(-int(e) // int(c)) * int(c)
    return n


def pyramid_work_bytes(zyx, n_levels, scale=(2, 2, 2)):
    """Bytes of the work buffer :meth:`DestripeEngine.pyramid_block` needs for ``n_levels`` levels (level 0 counted)."""
    lib = load_library()
    n = ctypes.c_size_t(0)
    if lib.dsx_pyramid_work_bytes_scale(*map(int, zyx), *pyramid_scale(scale), int(n_levels), ctypes.byref(n)) != 0:
        raise ValueError("pyramid_work_bytes: bad geometry {} / {} levels".format(tuple(zyx), n_levels))
    return int(n.value)


def volhist_ref(array, hist=None):
    """Host build of the voxel histogram (``dsx_volhist_ref``): the counts of a uint16 ``array`` of any shape as
    ``np.int64[65536]``; with ``hist`` (an ``np.int64[65536]`` of an earlier call) the counts are added to it."""
    lib = load_library()
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint16:
        raise ValueError("the voxel histogram takes uint16, got {}".format(a.dtype))
    if hist is None:
        hist = np.zeros(VOLHIST_BINS, np.int64)
    elif hist.dtype != np.int64 or hist.shape != (VOLHIST_BINS,) or not hist.flags["C_CONTIGUOUS"]:
        raise ValueError("hist must be a C-contiguous int64 array of {} bins".format(VOLHIST_BINS))
    rc = lib.dsx_volhist_ref(a.ctypes.data_as(ctypes.c_void_p), a.size, hist.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"volhist_ref failed").decode())
    return hist


def stack_rank_args(n, plane_elems, q_milli, valid_range):
    """``(n, plane_elems, [q, ...], lo, hi)`` of a stack-rank call as ints, inside the limits of ``include/dsx.h``;
    ``ValueError`` otherwise (raised before any library call)."""

    def whole(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("stack_rank: {} must be an integer, not {!r}".format(name, v))
        return int(v)

    n, plane_elems = whole("n", n), whole("plane_elems", plane_elems)
    if not (1 <= n <= STACK_RANK_MAX_PLANES):
        raise ValueError("stack_rank: 1 <= n <= {} planes, not {}".format(STACK_RANK_MAX_PLANES, n))
    if not (1 <= plane_elems <= STACK_RANK_MAX_ELEMS):
        raise ValueError("stack_rank: 1 <= plane_elems < 2^31, not {}".format(plane_elems))
    try:
        q = [whole("a quantile", v) for v in q_milli]
    except TypeError:
        raise ValueError("stack_rank: q_milli is a sequence of per-mille quantiles, not {!r}".format(q_milli)) from None
    if not (1 <= len(q) <= STACK_RANK_MAX_QUANTILES):
        raise ValueError("stack_rank: 1 <= len(q_milli) <= {}, not {}".format(STACK_RANK_MAX_QUANTILES, len(q)))
    if any(not (0 <= v <= 1000) for v in q):
        raise ValueError("stack_rank: a quantile is per-mille, 0 <= q <= 1000, not {!r}".format(q))
    try:
        lo, hi = valid_range
    except (TypeError, ValueError):
        raise ValueError("stack_rank: valid_range is (lo, hi), not {!r}".format(valid_range)) from None
    lo, hi = whole("lo", lo), whole("hi", hi)
    if not (0 <= lo <= hi <= 65535):
        raise ValueError("stack_rank: 0 <= lo <= hi <= 65535, not {!r}".format((lo, hi)))
    return n, plane_elems, q, lo, hi


def stack_rank_ref(stack, q_milli, valid_range=(0, 65535)):
    """Host build of :meth:`DestripeEngine.stack_rank` (``dsx_stack_rank_u16_ref``): ``stack`` is uint16 ``[n, ...]``,
    one plane per leading index.  Returns ``(out, valid)``: uint16 ``[len(q_milli), ...]`` and uint16 ``[...]``.  No GPU
    involved."""
    lib = load_library()
    a = np.ascontiguousarray(stack)
    if a.dtype != np.uint16 or a.ndim < 2:
        raise ValueError("stack_rank takes a uint16 stack [n, ...], got {} {}".format(a.dtype, a.shape))
    plane_shape = a.shape[1:]
    n, P, q, lo, hi = stack_rank_args(a.shape[0], int(np.prod(plane_shape)), q_milli, valid_range)
    out = np.empty((len(q),) + plane_shape, np.uint16)
    valid = np.empty(plane_shape, np.uint16)
    rc = lib.dsx_stack_rank_u16_ref(a.ctypes.data_as(ctypes.c_void_p), n, P, lo, hi, (ctypes.c_int * len(q))(*q), len(q),
                                    out.ctypes.data_as(ctypes.c_void_p), valid.ctypes.data_as(ctypes.c_void_p))  # fmt: skip
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"stack_rank_ref failed").decode())
    return out, valid


class NoSeenPixel(ValueError):
    """``dsx_flat_finish_*`` found ``valid == 0`` all over the image (``DSX_EVALUE``)."""


def gauss_taps(sigma):
    """``(radius, taps)`` of the native finish for a Gaussian of ``sigma`` pixels: ``radius = int(4 sigma + 0.5)`` and
    the centre and right half ``t_0 .. t_r`` (float64) of the taps ``flatfield_estimation.gaussian_smooth`` uses --
    ``exp(-0.5 / sigma^2 x^2)`` over ``x = -r .. r`` divided by its sum; that array is symmetric.  ``sigma == 0`` gives
    ``(0, [1.0])``.  ``0 <= sigma <= 64``, ``ValueError`` otherwise."""
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)):
        raise ValueError("gauss_taps: sigma must be a number, not {!r}".format(sigma))
    sigma = float(sigma)
    if not (0.0 <= sigma <= GAUSS_MAX_SIGMA):
        raise ValueError("gauss_taps: the native finish takes 0 <= sigma <= {}, not {!r}".format(GAUSS_MAX_SIGMA, sigma))
    if sigma == 0.0:
        return 0, np.ones(1, np.float64)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    taps = np.exp(-0.5 / (sigma * sigma) * x * x)
    taps /= taps.sum()
    return radius, np.ascontiguousarray(taps[radius:])


def _whole_extent(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError("{} must be an integer >= 1, not {!r}".format(what, v))
    return int(v)


def smooth_args(shape, taps, radius=None):
    """``(H, W, taps float64 [r + 1])`` of a smoothing call inside the limits of ``include/dsx.h``; ``ValueError``
    otherwise (raised before any library call).  The radius is ``len(taps) - 1``; a ``radius`` that is given must say
    the same."""
    try:
        H, W = shape
    except (TypeError, ValueError):
        raise ValueError("gauss_smooth: shape is (H, W), not {!r}".format(shape)) from None
    H, W = _whole_extent("gauss_smooth: H", H), _whole_extent("gauss_smooth: W", W)
    if H * W > FLAT_FINISH_MAX_ELEMS:
        raise ValueError("gauss_smooth: H * W < 2^31, not {} x {}".format(H, W))
    t = np.ascontiguousarray(taps, dtype=np.float64)
    if t.ndim != 1 or not (1 <= t.size <= GAUSS_MAX_RADIUS + 1) or not np.all(np.isfinite(t)):
        raise ValueError("gauss_smooth: taps are t_0 .. t_r, finite, 0 <= r <= {}".format(GAUSS_MAX_RADIUS))
    if radius is not None and (isinstance(radius, (bool, np.bool_)) or radius != t.size - 1):
        raise ValueError("gauss_smooth: radius {!r} and {} taps disagree (taps are t_0 .. t_radius)".format(radius, t.size))
    return H, W, t


def flat_finish_args(stored_shape, shape, n_q, taps, floor, radius=None):
    """``(Hs, Ws, H, W, n_q, taps, floor)`` of a finish call inside the limits of ``include/dsx.h``; ``ValueError``
    otherwise (raised before any library call)."""
    H, W, t = smooth_args(shape, taps, radius)
    try:
        Hs, Ws = stored_shape
    except (TypeError, ValueError):
        raise ValueError("flat_finish: stored_shape is (Hs, Ws), not {!r}".format(stored_shape)) from None
    Hs, Ws = _whole_extent("flat_finish: Hs", Hs), _whole_extent("flat_finish: Ws", Ws)
    if Hs < H or Ws < W or Hs * Ws > FLAT_FINISH_MAX_ELEMS:
        raise ValueError("flat_finish: the image {} must be the top-left crop of the stored planes {}, Hs * Ws < 2^31".format((H, W), (Hs, Ws)))
    if isinstance(n_q, (bool, np.bool_)) or n_q not in (1, 2):
        raise ValueError("flat_finish: n_q is 1 (flat) or 2 (flat, dark), not {!r}".format(n_q))
    if isinstance(floor, (bool, np.bool_)) or not isinstance(floor, (int, float, np.integer, np.floating)) or not (0.0 < float(floor) < 1e300):
        raise ValueError("flat_finish: floor must be positive and finite, not {!r}".format(floor))
    return Hs, Ws, H, W, int(n_q), t, float(floor)


def flat_finish_work_bytes(shape):
    """Bytes of the work buffer of :meth:`DestripeEngine.flat_finish` for an image ``(H, W)``."""
    H, W, _ = smooth_args(shape, [1.0])
    n = ctypes.c_size_t()
    if load_library().dsx_flat_finish_work_bytes(H, W, ctypes.byref(n)) != 0:
        raise ValueError("flat_finish_work_bytes: bad shape {!r}".format(shape))
    return int(n.value)


def gauss_smooth_ref(plane, taps, radius=None):
    """Host build of :meth:`DestripeEngine.gauss_smooth` (``dsx_gauss_smooth_f64_ref``): a float64 plane ``[H, W]`` and
    taps ``t_0 .. t_r``; returns the smoothed float64 plane.  No GPU involved."""
    lib = load_library()
    a = np.ascontiguousarray(plane)
    if a.dtype != np.float64 or a.ndim != 2:
        raise ValueError("gauss_smooth takes one float64 plane [H, W], got {} {}".format(a.dtype, a.shape))
    H, W, t = smooth_args(a.shape, taps, radius)
    tmp, out = np.empty_like(a), np.empty_like(a)
    vp = ctypes.c_void_p
    rc = lib.dsx_gauss_smooth_f64_ref(a.ctypes.data_as(vp), H, W, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      len(t) - 1, tmp.ctypes.data_as(vp), out.ctypes.data_as(vp))  # fmt: skip
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"gauss_smooth_ref failed").decode())
    return out


def flat_finish_ref(rank, valid, shape, taps, floor, radius=None):
    """Host build of :meth:`DestripeEngine.flat_finish` (``dsx_flat_finish_ref``): ``rank`` uint16 ``[n_q, Hs, Ws]``
    (flat, then dark), ``valid`` uint16 ``[Hs, Ws]``, the image ``shape = (H, W)`` their top-left crop.  Returns
    ``(flat, dark)`` as float32 ``[H, W]``, ``dark`` ``None`` when ``n_q == 1``.  :class:`NoSeenPixel` when ``valid`` is 0
    all over the image.  No GPU involved."""
    lib = load_library()
    R, v = np.ascontiguousarray(rank), np.ascontiguousarray(valid)
    if R.dtype != np.uint16 or R.ndim != 3 or v.dtype != np.uint16 or v.shape != R.shape[1:]:
        raise ValueError("flat_finish takes uint16 rank planes [n_q, Hs, Ws] and valid [Hs, Ws], got {} {} and {} {}".format(
            R.dtype, R.shape, v.dtype, v.shape))  # fmt: skip
    Hs, Ws, H, W, n_q, t, floor = flat_finish_args(R.shape[1:], shape, R.shape[0], taps, floor, radius)
    flat = np.empty((H, W), np.float32)
    dark = np.empty((H, W), np.float32) if n_q == 2 else None
    vp = ctypes.c_void_p
    rc = lib.dsx_flat_finish_ref(R.ctypes.data_as(vp), v.ctypes.data_as(vp), Hs, Ws, H, W, n_q,
                                 t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(t) - 1, floor,
                                 flat.ctypes.data_as(vp), dark.ctypes.data_as(vp) if n_q == 2 else None)  # fmt: skip
    if rc == -8:
        raise NoSeenPixel((lib.dsx_last_error(None) or b"").decode())
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"flat_finish_ref failed").decode())
    return flat, dark


def _project_geometry(zyx):
    try:
        Z, H, W = (int(n) for n in zyx)
    except (TypeError, ValueError):
        raise ValueError("projections: zyx is (Z, H, W), not {!r}".format(zyx))
    if Z < 0 or H <= 0 or W <= 0:
        raise ValueError("projections: Z >= 0, H > 0 and W > 0, not {!r}".format(tuple(zyx)))
    if max(Z, H, W) > PROJECT_MAX_EXTENT:
        raise ValueError("projections: more than {} rows, columns or planes of one call ({!r}); the uint32 sums could "
                         "overflow".format(PROJECT_MAX_EXTENT, tuple(zyx)))  # fmt: skip
    return Z, H, W


def projection_shapes(zyx):
    """``(name, shape, dtype)`` of the six projections of a ``zyx`` volume, in the order of ``dsx_projection``."""
    zyx = tuple(int(n) for n in zyx)
    return [(name, (zyx[axes[0]], zyx[axes[1]]), np.dtype(dtype)) for name, dtype, axes in PROJECTION_ARRAYS]


def project_work_bytes(zyx):
    """Bytes of the work buffer :meth:`DestripeEngine.project` needs for one call of ``zyx`` (``dsx_project_work_bytes``)."""
    Z, H, W = _project_geometry(zyx)
    n = ctypes.c_size_t(0)
    if load_library().dsx_project_work_bytes(Z, H, W, ctypes.byref(n)) != 0:
        raise ValueError("project_work_bytes: bad geometry {}".format((Z, H, W)))
    return int(n.value)


def project_ref(planes, acc=None, z_off=0):
    """Host build of the projections (``dsx_project_u16_ref``): ``planes`` is uint16 ``[Z, H, W]``.  Without ``acc`` the
    six arrays of that volume are returned as ``{name: array}`` (``PROJECTION_ARRAYS``).  With ``acc`` (such a dict for a
    volume of at least ``z_off + Z`` planes, zeros where nothing was added yet) the planes are rows ``z_off ..`` of it:
    those rows of the y / x arrays are written, the z arrays are combined; ``acc`` is returned."""
    lib = load_library()
    a = np.ascontiguousarray(planes)
    if a.dtype != np.uint16 or a.ndim != 3:
        raise ValueError("the projections take a uint16 [Z, H, W] array, got {} {}".format(a.dtype, a.shape))
    Z, H, W = _project_geometry(a.shape)
    z_off = int(z_off)
    if z_off < 0:
        raise ValueError("project_ref: z_off must not be negative")
    first = acc is None
    if first:
        if z_off:
            raise ValueError("project_ref: z_off needs the arrays it counts in (acc)")
        acc = {name: np.zeros(shape, dtype) for name, shape, dtype in projection_shapes(a.shape)}
    else:
        for name, shape, dtype in projection_shapes((z_off + Z, H, W)):
            arr = acc.get(name) if isinstance(acc, dict) else None
            if not (isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.ndim == 2 and arr.shape[1] == shape[1]
                    and (arr.shape[0] == H if name.endswith("_z") else arr.shape[0] >= shape[0]) and arr.flags["C_CONTIGUOUS"] and arr.flags["WRITEABLE"]):  # fmt: skip
                raise ValueError("project_ref: acc[{!r}] must be a C-contiguous {} array of at least {}".format(name, dtype, shape))
    table = _Projection(*[acc[name].ctypes.data for name, _, _ in PROJECTION_ARRAYS])
    rc = lib.dsx_project_u16_ref(a.ctypes.data_as(ctypes.c_void_p), Z, H, W, ctypes.byref(table), z_off, 1 if first else 0)
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"project_ref failed").decode())
    return acc


def digest_geometry(grid, chunks, valid):
    """``(grid, chunks, valid)`` of a digest call as three int triples; ``ValueError`` for what is no such geometry."""
    out = []
    for name, t in (("grid", grid), ("chunks", chunks), ("valid", valid)):
        t = tuple(int(x) for x in t)
        if len(t) != 3 or any(x < 1 or x >= 1 << 31 for x in t):
            raise ValueError("digest: {} must be three positive int32 values, got {}".format(name, t))
        out.append(t)
    return out


def brick_digest_ref(bricks, grid, chunks, valid):
    """Host build of the chunk digests (``dsx_brick_digest_u16_ref``): ``bricks`` holds ``prod(grid)`` bricks of
    ``chunks`` uint16 voxels back to back (any shape of that many elements; a view that starts at an odd element is
    fine), ``valid`` the voxels they cover along each axis.  Returns ``prod(grid)`` records of :data:`DIGEST_DTYPE`."""
    lib = load_library()
    n, c, v = digest_geometry(grid, chunks, valid)
    a = np.asarray(bricks)
    if a.dtype != np.uint16:
        raise ValueError("the digest takes uint16 voxels, got {}".format(a.dtype))
    if not a.flags["C_CONTIGUOUS"]:
        a = np.ascontiguousarray(a)
    count = n[0] * n[1] * n[2]
    out = np.zeros(count, DIGEST_DTYPE)
    brick = c[0] * c[1] * c[2]
    if brick > DIGEST_MAX_BRICK:
        raise ValueError("digest: a brick holds more than 2^31 voxels")
    if a.size < count * brick:
        raise ValueError("digest: {} voxels given, the grid holds {}".format(a.size, count * brick))
    rc = lib.dsx_brick_digest_u16_ref(a.ctypes.data_as(ctypes.c_void_p), *n, *c, *v, out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"brick_digest_ref failed").decode())
    return out


def streaks_blend_ref(x, f, b, t, crossover=10.0, bands="both", smoothing=0.0, flatfield=None, darkfield=None,
                      out_dtype=np.float32):
    """Host build of the options blend of a streaks plan (``dsx_streaks_blend_ref``) over one plane: ``x`` the plane,
    ``f`` / ``b`` the filtered foreground / background bands (``None`` for the band a one-sided ``bands`` leaves out),
    all ``[H, W]``; the arithmetic is the kernel's own.  No device call."""
    if bands not in STREAKS_BANDS:
        raise ValueError("bands must be 'both', 'fg' or 'bg', not {!r}".format(bands))
    smoothing = streaks_smoothing(smoothing)
    if (flatfield is None) != (darkfield is None):
        raise ValueError("flatfield and darkfield must be given together")
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.size == 0:
        raise ValueError("x must be one non-empty 2-D plane")
    planes = [None if p is None else np.ascontiguousarray(p, dtype=np.float32) for p in (f, b)]
    for p in planes:
        if p is not None and p.shape != x.shape:
            raise ValueError("the band planes must have the shape of x")
    flat = dark = None
    if flatfield is not None:
        flat, dark = _shading_planes(flatfield, darkfield, x.shape)
    opts = _StreaksOpts(STREAKS_BANDS[bands], smoothing, None if flat is None else flat.ctypes.data,
                        None if dark is None else dark.ctypes.data, 0 if dark is None else dark.shape[0],
                        0 if dark is None else dark.shape[1])  # fmt: skip
    out = np.empty(x.shape, dtype=out_dtype)
    rc = lib.dsx_streaks_blend_ref(x.ctypes.data, *[None if p is None else p.ctypes.data for p in planes],
                                   x.shape[0], x.shape[1], float(t), float(crossover), ctypes.byref(opts),
                                   out.ctypes.data, _dtype_code(out_dtype))  # fmt: skip
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"streaks_blend_ref failed").decode())
    return out


def pyramid_block_ref(planes, chunks, z0s=None, bricks=None, rows=None, scale=(2, 2, 2)):
    """Host build of :meth:`DestripeEngine.pyramid_block` (``dsx_pyramid_block_ref``): ``planes`` uint16 ``[Z, H, W]``
    -> one uint16 array ``[rows, nby, nbx, cz, cy, cx]`` per level ``1 .. len(chunks)``.  ``bricks``: arrays of an
    earlier call to write into (a chunk row filled by several blocks); fresh zeroed ones otherwise.  ``scale``: the window
    per axis, 1 or 2 each (``dsx_pyramid_block_scale_ref``)."""
    lib = load_library()
    scale = pyramid_scale(scale)
    a = np.ascontiguousarray(planes)
    if a.dtype != np.uint16 or a.ndim != 3:
        raise ValueError("the pyramid kernels take uint16 [Z, H, W] blocks")
    table = _pyramid_table(a.shape, chunks, z0s, [bricks is None] * len(chunks), rows, scale)
    out = []
    for i, ck in enumerate(chunks):
        g = table[i]
        shape = (g.rows, -(-pyramid_extent(a.shape[1], i + 1, scale[1]) // g.cy),
                 -(-pyramid_extent(a.shape[2], i + 1, scale[2]) // g.cx), g.cz, g.cy, g.cx)  # fmt: skip
        if bricks is None:
            out.append(np.zeros(shape, np.uint16))
        else:
            b = bricks[i]
            if b.dtype != np.uint16 or b.shape != shape or not b.flags["C_CONTIGUOUS"]:
                raise ValueError("level {}: bricks must be C-contiguous uint16 {}".format(i + 1, shape))
            out.append(b)
    n = len(chunks)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[o.ctypes.data for o in out])  # (a level with an empty share is not touched)
    rc = lib.dsx_pyramid_block_scale_ref(a.ctypes.data_as(ctypes.c_void_p), *a.shape, *scale, n + 1, table, ptrs)
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"pyramid_block_ref failed").decode())
    return out


def pyramid_bricks_ref(bricks, zyx, src_chunk, chunks, z0s=None, bricks_out=None, rows=None, scale=(2, 2, 2)):
    """Host build of :meth:`DestripeEngine.pyramid_bricks` (``dsx_pyramid_bricks_ref``): ``bricks`` uint16
    ``[nbz, nby, nbx] + src_chunk`` holding the block ``zyx`` -> one uint16 array ``[rows, nby, nbx, cz, cy, cx]`` per
    level ``1 .. len(chunks)``, the bytes :func:`pyramid_block_ref` gives for the dense block.  ``bricks_out``: arrays of
    an earlier call to write into; fresh zeroed ones otherwise.  ``scale``: the window per axis, 1 or 2 each
    (``dsx_pyramid_bricks_scale_ref``)."""
    lib = load_library()
    scale = pyramid_scale(scale)
    a = np.ascontiguousarray(bricks)
    zyx, src_chunk = tuple(int(v) for v in zyx), tuple(int(v) for v in src_chunk)
    if a.dtype != np.uint16 or len(zyx) != 3 or len(src_chunk) != 3 or min(src_chunk) <= 0:
        raise ValueError("the pyramid kernels take uint16 [Z, H, W] blocks")
    if a.size != src_brick_elems(zyx, src_chunk):
        raise ValueError("a {} block in chunks {} has {} voxels, not {}".format(zyx, src_chunk,
                                                                               src_brick_elems(zyx, src_chunk), a.size))  # fmt: skip
    table = _pyramid_table(zyx, chunks, z0s, [bricks_out is None] * len(chunks), rows, scale)
    out = []
    for i, ck in enumerate(chunks):
        g = table[i]
        shape = (g.rows, -(-pyramid_extent(zyx[1], i + 1, scale[1]) // g.cy),
                 -(-pyramid_extent(zyx[2], i + 1, scale[2]) // g.cx), g.cz, g.cy, g.cx)  # fmt: skip
        if bricks_out is None:
            out.append(np.zeros(shape, np.uint16))
        else:
            b = bricks_out[i]
            if b.dtype != np.uint16 or b.shape != shape or not b.flags["C_CONTIGUOUS"]:
                raise ValueError("level {}: bricks must be C-contiguous uint16 {}".format(i + 1, shape))
            out.append(b)
    n = len(chunks)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[o.ctypes.data for o in out])
    rc = lib.dsx_pyramid_bricks_scale_ref(a.ctypes.data_as(ctypes.c_void_p), *zyx, *src_chunk, *scale, n + 1, table, ptrs)
    if rc != 0:
        raise ValueError((lib.dsx_last_error(None) or b"pyramid_bricks_ref failed").decode())
    return out


# modes of the device Blosc encoder (DSX_ZENC_* of include/dsx.h): two zstd modes, and Blosc-LZ4 frames
ZENC_MODES = {"literals": 0, "runs": 1, "lz4": 3}


def zenc_mode(mode):
    try:
        return ZENC_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("unknown encoder mode {!r}: one of {}".format(mode, sorted(ZENC_MODES))) from None


def blosc_encode_ref(chunks, clevel=3, mode="literals"):
    """Host build of the device encoder (``dsx_blosc_encode_ref_ex``): ``chunks`` = uint16 array ``[n, ...]`` (one chunk
    per leading index) -> ``(frames: bytes, offsets: int64 [n + 1])``, byte-identical to ``Engine.blosc_encode_device``
    in the same ``mode`` (:data:`ZENC_MODES`)."""
    mode = zenc_mode(mode)
    lib = load_library()
    a = np.ascontiguousarray(chunks)
    if a.dtype != np.uint16:
        raise ValueError("the device Blosc encoders support uint16 (typesize 2) only")
    n = a.shape[0] if a.ndim else 0
    chunk_bytes = a.nbytes // n if n else 0
    frames = np.empty(n * (chunk_bytes + 16) + 1, np.uint8)
    offsets = np.zeros(n + 1, np.int64)
    rc = lib.dsx_blosc_encode_ref_ex(a.ctypes.data_as(ctypes.c_void_p), int(n), int(chunk_bytes), 2, int(clevel),
                                     frames.ctypes.data_as(ctypes.c_void_p), offsets.ctypes.data_as(ctypes.c_void_p),
                                     mode)  # fmt: skip
    if rc != 0:
        raise DsxError(rc, (lib.dsx_last_error(None) or b"blosc_encode_ref failed").decode())
    return frames[: offsets[-1]].tobytes(), offsets


def _io_read_frames(lib, ctx, paths, chunk_bytes, packed, tasks, threads, fill_value, routes, check, mode=0,
                    zlib_chunks=False):
    n = len(paths)
    assert packed.dtype == np.uint8 and packed.flags["C_CONTIGUOUS"] and tasks.dtype == TASK_DTYPE
    if routes is not None:
        assert routes.dtype == np.uint8 and routes.size >= n
    cp = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    pb, nt = ctypes.c_size_t(0), ctypes.c_int32(0)
    args = (ctx, cp, n, int(chunk_bytes), int(threads), int(fill_value), packed.ctypes.data_as(ctypes.c_void_p),
            packed.nbytes, tasks.ctypes.data_as(ctypes.c_void_p), int(tasks.size), ctypes.byref(pb), ctypes.byref(nt),
            routes.ctypes.data_as(ctypes.c_void_p) if routes is not None else None)  # fmt: skip
    check(lib.dsx_io_read_zlib_chunks(*args) if zlib_chunks else lib.dsx_io_read_frames_ex(*(args + (int(mode),))))
    return int(pb.value), int(nt.value)


def io_read_frames(paths, chunk_bytes, threads=4, fill_value=0, mode=0, zlib_chunks=False):
    """:meth:`DestripeEngine.io_read_frames` without an engine, into fresh buffers: ``(packed, tasks, routes)`` trimmed
    to what was read.  ``mode``: ``ZDEC_ZSTD``, ``ZDEC_ANY`` or ``ZDEC_ALL``; ``zlib_chunks``: plain-zlib chunk files."""
    lib = load_library()
    n = len(paths)
    packed = np.empty(n * (int(chunk_bytes) + 16) + 1, np.uint8)
    tasks = np.zeros(n * frame_tasks_per_chunk(chunk_bytes), TASK_DTYPE)
    routes = np.zeros(n, np.uint8)

    def check(rc):
        if rc != 0:
            raise DsxError(rc, (lib.dsx_last_error(None) or b"io_read_frames failed").decode())

    pb, nt = _io_read_frames(lib, None, paths, chunk_bytes, packed, tasks, threads, fill_value, routes, check, mode,
                             zlib_chunks)  # fmt: skip
    return packed[:pb], tasks[:nt], routes


def blosc_decode_ref(packed, tasks, out_bytes):
    """Host build of the device decoder (``dsx_blosc_decode_ref``): ``packed`` uint8 array, ``tasks`` ``TASK_DTYPE``
    array -> ``(out: uint8 [out_bytes], status: int32 per task)``, byte-identical to ``Engine.blosc_decode_device``."""
    lib = load_library()
    p = np.ascontiguousarray(packed, np.uint8)
    t = np.ascontiguousarray(tasks, TASK_DTYPE)
    out = np.zeros(int(out_bytes), np.uint8)
    status = np.zeros(len(t), np.int32)
    rc = lib.dsx_blosc_decode_ref(p.ctypes.data_as(ctypes.c_void_p), p.nbytes, t.ctypes.data_as(ctypes.c_void_p),
                                  len(t), out.ctypes.data_as(ctypes.c_void_p), out.nbytes,
                                  status.ctypes.data_as(ctypes.c_void_p))  # fmt: skip
    if rc != 0:
        raise DsxError(rc, (lib.dsx_last_error(None) or b"blosc_decode_ref failed").decode())
    return out, status
