/*
 * dsx.h  --  C ABI of the MI355X destripe engine (libdsx_hip.so).
 *
 * Drop-in boundary for ONE hot path of AllenNeuralDynamics/aind-smartspim-destripe: the per-plane
 * stripe filter.  Every entry point below replaces a piece of the reference's Python interface
 * (file:line relative to /root/reference/code/aind_smartspim_destripe/):
 *
 *   dsx_plan()        <- the arguments of filter_stripes()            filtering.py:417-424
 *                        (cells_config / no_cells_config dicts splatted into
 *                         log_space_fft_filtering(), filtering.py:139-145, 464, 467;
 *                         microscope_high_int, filtering.py:423, 462;
 *                         shadow_correction {flatfield, darkfield}, filtering.py:470-489)
 *   dsx_run_host()    <- the z-loop over planes of execute_worker()    zarr_destriper.py:319-327
 *                        and read_filter_save()                        destriper.py:194-200
 *   dsx_run_device()  <- same, operands already resident in HBM (what bench.py times)
 *   dsx_get_*()       <- per-level internals for parity tests (Otsu threshold filtering.py:190-193,
 *                        row medians filtering.py:200-202, cH / filtered cH filtering.py:186,217)
 *
 * Plain C types only; no torch / numpy types cross this boundary.  One context per GPU per
 * process; no global state; every call is synchronous unless stated.  All functions return 0
 * on success or a negative DSX_E* code; dsx_last_error() gives the message.
 *
 * Reference-side binding: see INTEGRATION.md (ctypes stub for filtering.py / zarr_destriper.py).
 */
#ifndef DSX_H
#define DSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSX_VERSION 100

/* error codes */
#define DSX_OK 0
#define DSX_EINVAL (-1)   /* bad argument (reference raises ValueError)            */
#define DSX_ENOPLAN (-2)  /* dsx_run_* before dsx_plan                              */
#define DSX_EHIP (-3)     /* HIP runtime error                                      */
#define DSX_ENOMEM (-4)   /* device or host allocation failed                       */
#define DSX_ELIMIT (-5)   /* plane exceeds an implementation limit                  */
#define DSX_ECOMM (-6)    /* RCCL error / communicator not initialised              */
#define DSX_EIO (-7)      /* chunk file could not be read / written                  */
#define DSX_EVALUE (-8)   /* a float32 pixel is NaN, infinite or <= -1: the reference raises ValueError from
                             numpy.histogram inside threshold_otsu (filtering.py:188); dsx_run_host only      */

/* plane element types */
#define DSX_U16 0 /* uint16 pixels (TIFF path, destriper.py:172-200)                 */
#define DSX_F32 1 /* float32 pixels (Zarr path, zarr_destriper.py:1049)              */

/* wavelet ids: db3 is the production setting (run_capsule.py:374-390) and has its own kernels; any other
 * wavelet the reference's config may name (pywt.wavedec2(..., wavelet=...), filtering.py:176) is handed over
 * as its filter bank with dsx_set_wavelet and selected with DSX_WAVELET_BANK                              */
#define DSX_WAVELET_DB3 3
#define DSX_WAVELET_BANK 0

/* stage buffers for dsx_get_level() */
#define DSX_STAGE_APPROX 0 /* aa_l (before the inverse pass overwrites it with c_l)   */
#define DSX_STAGE_DETAIL 1 /* da_l == cH_l, or Delta_l once the row filter has run    */

typedef struct dsx_ctx dsx_ctx;

/* One config dict of the reference: {"wavelet","level","sigma","max_threshold"}. */
typedef struct dsx_cfg {
  int32_t wavelet;     /* DSX_WAVELET_DB3 or DSX_WAVELET_BANK; both configs the same   */
  int32_t level;       /* -1 == None (maximum level), 0 == filter is the identity + 2 */
  float sigma;         /* > 0                                                         */
  float max_threshold; /* upper bound of the Otsu threshold                           */
} dsx_cfg;

/* Geometry of a planned plane (filled by dsx_plan_info). */
typedef struct dsx_plan_info_t {
  int32_t height, width;         /* input plane                                       */
  int32_t out_height, out_width; /* result plane: H + (H & 1) when any level runs     */
  int32_t levels;                /* decomposition depth actually run (max of both cfg) */
  int32_t level_h[16], level_w[16]; /* cH shape per level, index 0 == finest           */
  int32_t fft_len[16];           /* transform length used by the row filter per level  */
  int32_t fft_halo[16];          /* periodic halo K (0 == direct length-w transform)   */
  int32_t max_batch;             /* planes per cohort                                  */
  uint64_t workspace_bytes;      /* device workspace                                   */
} dsx_plan_info_t;

/* ---- context ------------------------------------------------------------------------------ */
int dsx_init(int device, dsx_ctx** out_ctx);
void dsx_destroy(dsx_ctx* ctx);
const char* dsx_last_error(const dsx_ctx* ctx); /* ctx may be NULL: last dsx_init error */
int dsx_device_count(void);

/* ---- plan: everything filter_stripes() takes besides the plane itself --------------------- */
/* flat / dark: host float32 planes (flat[H*W] row-major, dark[dark_h*dark_w] row-major, cropped
 * to the plane as flatfield_correction() does, filtering.py:377) or NULL for no shading.      */
int dsx_plan(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_cfg* cells_config,
             const dsx_cfg* no_cells_config, double microscope_high_int, const float* flat,
             const float* dark, int dark_h, int dark_w);
int dsx_plan_info(const dsx_ctx* ctx, dsx_plan_info_t* info);
/* The four filters of a pywt.Wavelet (dec_lo, dec_hi, rec_lo, rec_hi; `len` taps each, even, 2 ... 104) for
 * plans whose configs carry DSX_WAVELET_BANK: what the reference passes by name to pywt.wavedec2 / waverec2
 * (filtering.py:176, 221).  Mode 'symmetric', perfect-reconstruction banks only (the engine reconstructs the
 * correction, not the plane).  Takes effect at the next dsx_plan.                                          */
int dsx_set_wavelet(dsx_ctx* ctx, const double* dec_lo, const double* dec_hi, const double* rec_lo,
                    const double* rec_hi, int len);
/* Vertical stripes (pystripe's `rotate` switch of read_filter_save / batch_filter): sticky context state like the
 * filter bank, read by the next dsx_plan / dsx_plan_streaks*.  A plan made with it on computes, per plane,
 *     np.rot90( F(np.rot90(x)), -1 )          np.rot90(x)[i, j] == x[j, W - 1 - i], shape [W, H]
 * with F the same plan without it: the plan takes the caller's height and width and plans the chain for
 * (width, height) -- sigma / min(H, W), the level count, the odd-size growth and the even padding are those of the
 * rotated plane -- and dsx_run_host / dsx_run_device take and return planes in the caller's orientation: every stream
 * part of a cohort turns its planes ahead of its first kernel and its result back behind its last one
 * (csrc/dsx_rot90.h), through two buffers of max_batch planes the plan owns.  flat / dark of dsx_plan,
 * dsx_plan_streaks_opts and dsx_set_shading_device stay in the caller's orientation (the dark is cropped to the plane,
 * then both are turned by the plan).  dsx_plan_info reports height / width / out_height / out_width of the caller's
 * plane; level_h / level_w, dsx_get_level and dsx_get_thresholds are those of the rotated chain.  cfg_used and the
 * streaks threshold do not depend on the orientation.  A caller's height above the row filter's width limit (36 856)
 * is DSX_ELIMIT.  DSX_GRAPH=1 runs such a plan eagerly.  Off (the default): nothing changes, no kernel is added and no
 * buffer is allocated. */
int dsx_set_rotate(dsx_ctx* ctx, int on);
/* The quarter turn on its own: n planes [H, W] -> [W, H] of dtype (DSX_U16 / DSX_F32), dir +1 == np.rot90(x),
 * -1 == np.rot90(x, -1), per plane.  Device pointers, not in place, asynchronous on the context stream.
 * dsx_rot90_ref: the same index map on the host (host pointers, synchronous, no context: dsx_last_error(NULL)). */
int dsx_rot90_device(dsx_ctx* ctx, const void* d_src, void* d_dst, int dtype, int n, int H, int W, int dir);
int dsx_rot90_ref(const void* src, void* dst, int dtype, int n, int H, int W, int dir);
/* Same, with the shading planes already in device memory (e.g. after an RCCL broadcast). */
int dsx_set_shading_device(dsx_ctx* ctx, const float* d_flat, const float* d_dark, int dark_h,
                           int dark_w);
/* Device address + size of the constant blob (twiddles, gain tables, shading) so that a host
 * program can broadcast it between ranks (RCCL) instead of rebuilding it per rank.              */
int dsx_constants_device(const dsx_ctx* ctx, void** d_ptr, size_t* bytes);

/* ---- run ---------------------------------------------------------------------------------- */
/* n planes, C-order [n, H, W] in, [n, H', W'] out.  out_dtype DSX_F32: exp(y)+1 (after shading
 * if planned, before the integer cast); DSX_U16: clip to [0, 65535] and truncate.
 * cfg_used (nullable): per plane 1 == cells_config, 0 == no_cells_config (0 throughout when neither
 * config runs a decomposition level: the result is image + 2 either way and no statistic is made). */
int dsx_run_host(dsx_ctx* ctx, const void* in, int in_dtype, int n, void* out, int out_dtype,
                 int32_t* cfg_used);
/* Device pointers; asynchronous on the context stream (call dsx_sync).  d_cfg_used nullable. */
int dsx_run_device(dsx_ctx* ctx, const void* d_in, int in_dtype, int n, void* d_out,
                   int out_dtype, int32_t* d_cfg_used);
int dsx_sync(dsx_ctx* ctx);
/* With DSX_GRAPH=1 in the environment, cohorts that run as ONE part (fewer than 32 planes: the per-slice calls of
 * filter_stripes, filtering.py:417, and small batches) are replayed as a HIP graph from the third call with the
 * same buffers, count and element types on (first call eager, second captured): one graph launch instead of ~30
 * kernel launches.  Off by default: measured 5-8 % slower than eager launches on ROCm 7.2.
 * Counters for tests / diagnosis.                                                                           */
int dsx_graph_stats(const dsx_ctx* ctx, uint64_t* launches, uint64_t* captures);
/* Launches of the packed coarse row filter (k_rowfilter_pack: several row pairs per wave) this context has enqueued;
 * 0 throughout with DSX_NO_ROW_PACK=1.  Counter for tests / diagnosis.                                         */
int dsx_row_pack_launches(const dsx_ctx* ctx, uint64_t* launches);

/* ---- device memory + timing helpers for host programs without a GPU array library --------- */
int dsx_malloc(dsx_ctx* ctx, size_t bytes, void** d_ptr);
int dsx_free(dsx_ctx* ctx, void* d_ptr);
int dsx_memcpy_h2d(dsx_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int dsx_memcpy_d2h(dsx_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int dsx_memcpy_d2d(dsx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* Pinned host staging + copies on their own streams, so that a caller can overlap the upload of
 * block k+1 and the download of block k-1 with the kernels of block k -- the role the reference's
 * producer / consumer queue plays on CPU cores (zarr_destriper.py:797-906, 1138-1172).
 * stream ids: DSX_STREAM_COMPUTE is the context stream every dsx_run_device / re-tiling call uses. */
#define DSX_STREAM_COMPUTE 0
#define DSX_STREAM_UPLOAD 1
#define DSX_STREAM_DOWNLOAD 2
int dsx_malloc_host(dsx_ctx* ctx, size_t bytes, void** h_ptr);
int dsx_free_host(dsx_ctx* ctx, void* h_ptr);
int dsx_memcpy_h2d_async(dsx_ctx* ctx, void* d_dst, const void* src, size_t bytes, int stream_id);
int dsx_memcpy_d2h_async(dsx_ctx* ctx, void* dst, const void* d_src, size_t bytes, int stream_id);
/* Work submitted to `waiter` after this call starts only when everything submitted to `signaller`
 * before it has finished (event record + stream wait; nothing blocks the host).                 */
int dsx_stream_wait(dsx_ctx* ctx, int waiter, int signaller);
int dsx_stream_sync(dsx_ctx* ctx, int stream_id);
/* Host-visible completion marks, slots 0..7: record on a stream, later block the host until everything
 * submitted to that stream before the record has finished (staging buffer k may be refilled / written out). */
int dsx_event_record(dsx_ctx* ctx, int slot, int stream_id);
int dsx_event_sync(dsx_ctx* ctx, int slot);
/* HIP events on the context stream: start, stop -> elapsed milliseconds. */
int dsx_timer_start(dsx_ctx* ctx);
int dsx_timer_stop(dsx_ctx* ctx, float* ms);
/* Per-kernel-class device time of the runs since the last reset (HIP events around every
 * launch; slows the pipeline down, for diagnosis only).  names: NUL-separated list.           */
int dsx_profile_enable(dsx_ctx* ctx, int on);
int dsx_profile_read(dsx_ctx* ctx, int max_classes, float* ms, int32_t* launches,
                     const char** names, int* n_classes);

/* ---- data formats either side of the filter ------------- */
/* Zarr chunk ("brick") order <-> dense planes, uint16, device pointers, asynchronous on the
 * context stream.  Replaces the NumPy gather of (1,1,64,128,128) chunks into a block and the
 * scatter of the filtered block back into chunks (zarr_destriper.py:1066-1074 and :336).
 * d_bricks: [nbz][nby][nbx][cz][cy][cx], every brick full-sized as zarr stores it
 * (nb* = ceil over the axis; nbz = ceil((z0 + Z) / cz)); d_planes: dense [Z][H][W]; z0: position
 * of plane 0 inside the brick grid.  planes_to_bricks writes 0 (the fill value) where a brick
 * sticks out of the stack.                                                                    */
int dsx_bricks_to_planes_u16(dsx_ctx* ctx, const void* d_bricks, void* d_planes, int Z, int H,
                             int W, int cz, int cy, int cx, int z0);
int dsx_planes_to_bricks_u16(dsx_ctx* ctx, const void* d_planes, void* d_bricks, int Z, int H,
                             int W, int cz, int cy, int cx, int z0);
/* One 2x2x2 windowed-mean pyramid level, uint16 [Z,Y,X] -> [Z/2,Y/2,X/2] (odd trailing voxels are
 * cropped), value = floor(sum of 8 / 8): compute_pyramid(), zarr_destriper.py:365-407, i.e.
 * xarray_multiscale.reducers.windowed_mean + preserve_dtype.  Asynchronous on the context stream. */
int dsx_downsample2_u16(dsx_ctx* ctx, const void* d_src, void* d_dst, int Z, int Y, int X);

/* The pyramid levels of one filtered block, computed from the block where it lies and stored in chunk order: what
 * compute_pyramid (zarr_destriper.py:365-407) and the level loop of compute_multiscale (:746-782) produce for the
 * voxels under this block, without reading level 0 back.  d_planes: dense [Z][H][W] uint16 whose plane 0 lies at a
 * multiple of 2^(n_levels - 1) in the volume.  n_levels counts level 0; levels[l - 1] / d_bricks[l - 1] describe level
 * l = 1 .. n_levels - 1, whose share of the block is (Z >> l, H >> l, W >> l) -- every level the floor(sum of 8 / 8)
 * of the TRUNCATED previous one, trailing odd planes / rows / columns cropped per level.  A level (and all below it)
 * with an empty share is skipped.  d_bricks[l - 1]: [rows][nby][nbx][cz][cy][cx] with nb* = ceil((H or W) >> l / c*);
 * positions outside the level's volume are not written, so the first block of a chunk row sets `zero`.
 * Levels 1 and 2 come from one kernel that reads the block once; levels >= 3 from one plain kernel each, through
 * d_work (dsx_pyramid_work_bytes; may be NULL when that is 0).  Asynchronous on the context stream.
 * dsx_pyramid_block_ref: the host build of the same arithmetic (host pointers, synchronous, identical output). */
typedef struct dsx_pyramid_level {
  int32_t cz, cy, cx; /* chunk shape of the level, already clamped to the level's volume */
  int32_t rows;       /* chunk rows the level's brick buffer holds */
  int32_t z0;         /* first plane of this block's share inside that brick grid */
  int32_t zero;       /* non-zero: the whole brick buffer is zeroed first */
} dsx_pyramid_level;
int dsx_pyramid_work_bytes(int Z, int H, int W, int n_levels, size_t* bytes);
int dsx_pyramid_block_u16(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, int n_levels,
                          const dsx_pyramid_level* levels, void* const* d_bricks, void* d_work, size_t work_bytes);
int dsx_pyramid_block_ref(const void* planes, int Z, int H, int W, int n_levels, const dsx_pyramid_level* levels,
                          void* const* bricks);
/* The same levels from a block that is still in the chunk order it was stored in -- a decoded level-0 block of a
 * finished store, for the stand-alone pyramid (compute_pyramid, zarr_destriper.py:365-407; level loop of
 * compute_multiscale, :746-782) -- without dsx_bricks_to_planes_u16 in front.  d_src_bricks:
 * [nbz][nby][nbx][src_cz][src_cy][src_cx] uint16, every brick full-sized, nb* = ceil((Z, H, W) / src_c*); plane 0 of
 * the block is plane 0 of the brick grid (the block starts on a source chunk boundary).  Bricks that stick out of
 * [Z, H, W] hold whatever the store held there: those positions are never read.  levels / d_bricks / d_work, `zero`,
 * `rows`, `z0`, the outputs and the refusals are dsx_pyramid_block_u16's.  Asynchronous on the context stream.
 * dsx_pyramid_bricks_ref: the host build (host pointers, synchronous, identical output). */
int dsx_pyramid_bricks_u16(dsx_ctx* ctx, const void* d_src_bricks, int Z, int H, int W, int src_cz, int src_cy,
                           int src_cx, int n_levels, const dsx_pyramid_level* levels, void* const* d_bricks,
                           void* d_work, size_t work_bytes);
int dsx_pyramid_bricks_ref(const void* src_bricks, int Z, int H, int W, int src_cz, int src_cy, int src_cx,
                           int n_levels, const dsx_pyramid_level* levels, void* const* bricks);
/* The same calls with a scale factor per axis (compute_pyramid(scale_axis=...), compute_multiscale(scale_factor=...),
 * zarr_destriper.py:365-407, 677-794), for anisotropic volumes: fz, fy, fx are 1 or 2 each and not all 1, anything else
 * is DSX_EINVAL.  Level l has the extent of level l - 1 divided by the factor per axis (trailing voxels cropped), every
 * voxel floor(sum of the fz x fy x fx window of the TRUNCATED previous level / (fz fy fx)); an axis with factor 1 keeps
 * its extent.  A block's plane 0 lies at a multiple of fz^(n_levels - 1).  With (2, 2, 2) each call IS the one above.
 * With any other scale every level is one kernel from the dense previous level, so d_work holds the dense levels
 * 1 .. n_levels - 2 (dsx_pyramid_work_bytes_scale) and is needed from two levels on; more than 65535 rows or planes of
 * a level is DSX_ELIMIT.  dsx_downsample_u16: one dense level, [Z,Y,X] -> [Z/fz,Y/fy,X/fx]. */
int dsx_downsample_u16(dsx_ctx* ctx, const void* d_src, void* d_dst, int Z, int Y, int X, int fz, int fy, int fx);
int dsx_pyramid_work_bytes_scale(int Z, int H, int W, int fz, int fy, int fx, int n_levels, size_t* bytes);
int dsx_pyramid_block_scale_u16(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, int fz, int fy, int fx,
                                int n_levels, const dsx_pyramid_level* levels, void* const* d_bricks, void* d_work,
                                size_t work_bytes);
int dsx_pyramid_block_scale_ref(const void* planes, int Z, int H, int W, int fz, int fy, int fx, int n_levels,
                                const dsx_pyramid_level* levels, void* const* bricks);
int dsx_pyramid_bricks_scale_u16(dsx_ctx* ctx, const void* d_src_bricks, int Z, int H, int W, int src_cz, int src_cy,
                                 int src_cx, int fz, int fy, int fx, int n_levels, const dsx_pyramid_level* levels,
                                 void* const* d_bricks, void* d_work, size_t work_bytes);
int dsx_pyramid_bricks_scale_ref(const void* src_bricks, int Z, int H, int W, int src_cz, int src_cy, int src_cx, int fz,
                                 int fy, int fx, int n_levels, const dsx_pyramid_level* levels, void* const* bricks);

/* Exact histogram of the uint16 voxels a pass writes, for the display window of the OME-NGFF metadata: the reference
 * says the window should be da.percentile(image_data, (0.1, 95)) and hard-codes (0.0, 350.0) because of the cost
 * (zarr_destriper.py:722-726); a histogram taken while the filtered planes lie in device memory makes it exact for one
 * more read of them (csrc/dsx_volhist.h).  The context owns 65 536 uint64 bins that accumulate over calls.  n == 0 is a
 * no-op; a NULL (or odd) pointer with n > 0, and add / get before the first reset, are DSX_EINVAL; n >= 2^32 in one call
 * is DSX_ELIMIT (the block-local counters are 32 bits wide).  dsx_destroy frees the bins; no plan call touches them. */
/* zarr_destriper.py:722-726: allocate the bins on first use and zero them (asynchronous on the context stream). */
int dsx_volhist_reset(dsx_ctx* ctx);
/* zarr_destriper.py:722-726: count n contiguous uint16 voxels in device memory (2-byte aligned; asynchronous on the
 * context's current stream). */
int dsx_volhist_add_device(dsx_ctx* ctx, const void* d_vox, size_t n);
/* zarr_destriper.py:722-726: the 65 536 counts to the host; synchronises that stream. */
int dsx_volhist_get(dsx_ctx* ctx, uint64_t* hist);
/* zarr_destriper.py:722-726: the host build -- adds the counts of n host voxels into hist (65 536 bins). */
int dsx_volhist_ref(const void* vox, size_t n, uint64_t* hist);

/* Per-pixel order statistics of a stack of uint16 planes (csrc/dsx_stackrank.h): what this project's estimator of the
 * retrospective flat fields needs from the device.  The reference fits them with BaSiC over destriped sample tiles
 * (flatfield_estimation.py:15-52, 125-196); here the destriped samples lie in device memory behind the filter and the
 * flat is a smoothed per-pixel quantile of them (aind_smartspim_destripe_amd/flatfield_estimation.py).
 *   planes: n dense planes of plane_elems uint16 each (2-byte aligned; plane_elems may be odd)
 *   per pixel p: V = the x[j, p] with lo <= x <= hi, m = |V|; valid[p] = m (valid may be NULL);
 *   out[i, p] = the k-th smallest element of V, 0-based, k = (q_milli[i] * (m - 1)) / 1000 in integer arithmetic,
 *   and 0 where m == 0.  out is uint16 [n_q][plane_elems].
 * 1 <= n <= 512, 1 <= n_q <= 4, 1 <= plane_elems < 2^31, 0 <= lo <= hi <= 65535, 0 <= q_milli[i] <= 1000, non-NULL
 * planes, q_milli and out: anything else is DSX_EINVAL, before anything is launched.  Integers only: the two builds agree
 * exactly. */
/* flatfield_estimation.py:43-50: device pointers, the stack is read once; asynchronous on the context stream. */
int dsx_stack_rank_u16_device(dsx_ctx* ctx, const void* d_planes, int n, size_t plane_elems, int lo, int hi,
                              const int* q_milli, int n_q, void* d_out /* u16 [n_q][plane_elems] */,
                              void* d_valid /* u16 [plane_elems], may be NULL */);
/* flatfield_estimation.py:43-50: the host build, plain C++ (host pointers, synchronous). */
int dsx_stack_rank_u16_ref(const void* planes, int n, size_t plane_elems, int lo, int hi, const int* q_milli, int n_q,
                           void* out, void* valid);

/* The finish of a retrospective flat on the device (csrc/dsx_smooth.h): what flatfield_estimation.py of this project does
 * to the rank planes of dsx_stack_rank_u16_* -- a masked median fill, scipy's Gaussian and a division by the mean -- where
 * those planes lie.  It stands in for the BaSiC fit of the reference (flatfield_estimation.py:15-52).  The contract
 * ("native finish") fixes every float64 operation, so the device and the host build agree bit for bit:
 *   taps   radius r and t_0 .. t_r, the centre and the right half of the normalised, symmetric Gaussian (0 <= r <= 256)
 *   fold   m(j): j' = j mod 2n, non-negative; m = j' if j' < n else 2n - 1 - j'      (np.pad(mode="symmetric"))
 *   smooth along an axis of length n: acc = t_0 * a[i]; for k = 1 .. r: acc = fma(t_k, a[m(i - k)] + a[m(i + k)], acc);
 *          axis 0 first, then axis 1
 *   fill   per rank plane, over the H x W top-left crop of the stored Hs x Ws plane: seen = valid > 0; fill = the median
 *          of R[seen] (the middle value, or the mean of the two middle values: exact from a 65 536-bin count);
 *          a[y, x] = seen ? double(R) : fill
 *   mean   S = the smoothed flat plane, row-major, N = H * W: p_j = the sum of S[i] over i = j (mod 4096) in increasing
 *          i from 0.0; mean = (p_0 + p_1 + ... + p_4095, left to right) / N
 *   result flat = float32(q < floor ? floor : q), q = S / mean (IEEE division); dark = float32(S_dark) when n_q == 2
 * 1 <= H, W, H * W < 2^31 (and Hs >= H, Ws >= W, Hs * Ws < 2^31), 0 <= radius <= 256, n_q 1 or 2, floor positive and
 * finite, non-NULL aligned pointers: anything else is DSX_EINVAL before anything is launched. */
/* flatfield_estimation.py:15-52 (the smoothing of this project's estimator): the two passes alone on float64 [H][W]
 * device planes; d_tmp is a third plane of that size, d_out may be d_in.  Asynchronous on the context stream. */
int dsx_gauss_smooth_f64_device(dsx_ctx* ctx, const void* d_in, int H, int W, const double* taps /* host, [radius + 1] */,
                                int radius, void* d_tmp, void* d_out);
/* flatfield_estimation.py:15-52: the host build of the two passes, plain C++ (host pointers, synchronous). */
int dsx_gauss_smooth_f64_ref(const void* in, int H, int W, const double* taps, int radius, void* tmp, void* out);
/* Bytes of the work buffer dsx_flat_finish_device takes for an H x W image. */
int dsx_flat_finish_work_bytes(int H, int W, size_t* bytes);
/* flatfield_estimation.py:15-52: fill, smooth, mean and result of the contract above, from d_rank (uint16
 * [n_q][Hs * Ws]: flat, then dark) and d_valid (uint16 [Hs * Ws]) to d_flat (float32 [H][W]) and d_dark (float32 [H][W];
 * not touched and may be NULL when n_q == 1).  d_work: dsx_flat_finish_work_bytes bytes, 16-byte aligned.  The launches
 * run on the context stream with no host round trip between them; the call then reads the seen count once and returns
 * DSX_EVALUE when no pixel of the image is seen (the results then hold nothing of use). */
int dsx_flat_finish_device(dsx_ctx* ctx, const void* d_rank, const void* d_valid, int Hs, int Ws, int H, int W, int n_q,
                           const double* taps /* host, [radius + 1] */, int radius, double floor, void* d_flat, void* d_dark,
                           void* d_work);
/* flatfield_estimation.py:15-52: the host build of the finish, plain C++ (host pointers; DSX_EVALUE as above, with
 * nothing written). */
int dsx_flat_finish_ref(const void* rank, const void* valid, int Hs, int Ws, int H, int W, int n_q, const double* taps,
                        int radius, double floor, void* flat, void* dark);

/* QC projections of a pass: the three maximum-intensity projections of a uint16 volume and the three sum projections,
 * whose row sums before and after the filter are the stripe signature and what became of it (csrc/dsx_project.h).  The
 * reference leaves only a resource plot in its results folder (zarr_destriper.py:1202-1211).  A volume v[., H, W]
 * arrives in z blocks: planes = Z dense planes (2-byte aligned), which are rows z_off .. z_off + Z - 1 of the volume.
 *   max_z uint16 [H, W], sum_z uint64 [H, W]: over z -- overwritten when first != 0, combined with their content otherwise
 *   max_y uint16 [., W], sum_y uint32 [., W]: over y -- rows z_off .. z_off + Z - 1 are written, no other row is touched
 *   max_x uint16 [., H], sum_x uint32 [., H]: over x -- likewise
 * All integers, exact, independent of the order of the blocks.  H, W > 0, Z >= 0, z_off >= 0, anything else is
 * DSX_EINVAL; H, W or Z above 65 536 is DSX_ELIMIT (the uint32 sums); Z == 0 is a no-op; with Z > 0 a NULL planes
 * pointer, table, table member or work buffer and an odd planes pointer are DSX_EINVAL, all before anything is launched.
 * dsx_project_u16_device: device pointers, one read of the planes, asynchronous on the context stream; d_work holds
 * dsx_project_work_bytes(Z, H, W) bytes (4-byte aligned) and may be reused by the next call on the stream.
 * dsx_project_u16_ref: the host build of the same arithmetic (host pointers, synchronous, no work buffer). */
typedef struct dsx_projection {
  uint16_t* max_z; uint64_t* sum_z;
  uint16_t* max_y; uint32_t* sum_y;
  uint16_t* max_x; uint32_t* sum_x;
} dsx_projection;
int dsx_project_work_bytes(int Z, int H, int W, size_t* bytes);
int dsx_project_u16_device(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, const dsx_projection* p, int z_off,
                           int first, void* d_work);
int dsx_project_u16_ref(const void* planes, int Z, int H, int W, const dsx_projection* p, int z_off, int first);

/* Content digests of the chunks a pass writes (csrc/dsx_digest.h): neither the Blosc frames nor the zstd frames of a
 * store carry a checksum, so a chunk that decodes to the wrong voxels raises nothing; a record per chunk, taken while
 * the voxels lie in device memory in chunk order, lets a later pass over the store say "these are the voxels the filter
 * produced" (integrity.py).  bricks: n0 * n1 * n2 bricks of (c0, c1, c2) uint16 voxels back to back, in C order of the
 * grid (2-byte aligned) -- what the re-tiling kernels, the pyramid kernels and the decoders leave.  (v0, v1, v2): the
 * valid voxels the buffer covers along each axis from its chunk-aligned origin, (n_a - 1) * c_a < v_a <= n_a * c_a, so
 * brick g has extents e_a = min(c_a, v_a - g_a * c_a); padding never enters.  out: uint64 [n0 * n1 * n2][3] (8-byte
 * aligned), per brick {count, sum, wsum}: with m(k) splitmix64's output over (k + 1) * 0x9E3779B97F4A7C15, made odd,
 *   count = e0 * e1 * e2,  sum = SUM v,  wsum = SUM_r m(r) * SUM_{i2 < e2} v[r, i2] * m(2^32 + i2)    (mod 2^64)
 * over the valid voxels, r = i0 * c1 + i1 the row index in the FULL chunk.  Exact integers: device, host build and a
 * NumPy restatement agree bit for bit.  Every weight is odd: changing one voxel changes wsum.  Not cryptographic.
 * Shapes below 1, bricks above 2^31 voxels, rows above 2^30, extents that do not end inside the last brick, NULL or
 * misaligned pointers and an unknown stream id are DSX_EINVAL before anything is launched.
 * The device call zeroes the records and launches on stream `stream_id` (DSX_STREAM_*); it never synchronises.
 * The ref call is the host build of the same arithmetic (host pointers, synchronous). */
int dsx_brick_digest_u16_device(dsx_ctx* ctx, const void* d_bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0,
                                int v1, int v2, void* d_out, int stream_id);
int dsx_brick_digest_u16_ref(const void* bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0, int v1, int v2,
                             void* out);

/* Host side of the chunk map: n Zarr chunk files <-> memory (normally the pinned staging buffers) on
 * `threads` native threads -- what zarr / numcodecs do under the reference's worker processes
 * (zarr_destriper.py:336, 1042-1074).  codec: raw chunks, zlib streams, or Blosc frames -- the production
 * arrays are Blosc(cname="zstd", clevel=3, shuffle=SHUFFLE) (zarr_destriper.py:1066-1074); the c-blosc 1.x
 * container is restated in csrc/dsx_io.h (zstd / lz4 / blosclz / zlib inside, byte or bit shuffle; libzstd.so.1
 * and liblz4.so.1 are dlopen'ed), pinned by frames of the real c-blosc 1.21.0 (tests/golden/blosc_frames.npz) and by
 * decoding this writer's frames with that library (tests/test_blosc.py).  A missing chunk reads as the
 * 16-bit fill value; writes go to "<path>.tmp" and are renamed.  bytes[i] is the decompressed chunk size.
 * Synchronous; no GPU involved (ctx may be NULL: the message of a failure is then read with
 * dsx_last_error(NULL)).                                                                              */
#define DSX_CODEC_RAW 0
#define DSX_CODEC_ZLIB 1
#define DSX_CODEC_BLOSC 2
int dsx_io_read_chunks(dsx_ctx* ctx, const char* const* paths, void* const* dst, const size_t* bytes,
                       int n, int threads, int codec, uint16_t fill_value);
/* zlib_level < 0: raw chunks, otherwise zlib streams of that level */
int dsx_io_write_chunks(dsx_ctx* ctx, const char* const* paths, const void* const* src,
                        const size_t* bytes, int n, int threads, int zlib_level);
/* Blosc frames with zstd inside: clevel 0 ... 9 (Blosc's scale), typesize = element size, shuffle 0 / 1 */
int dsx_io_write_chunks_blosc(dsx_ctx* ctx, const char* const* paths, const void* const* src,
                              const size_t* bytes, int n, int threads, int clevel, int typesize, int shuffle);
/* One frame in memory (what numcodecs.Blosc.decode / .encode do for one chunk); errors: dsx_last_error(NULL).
 * A frame never exceeds bytes + 16.                                                                    */
int dsx_blosc_decode(const void* frame, size_t frame_bytes, void* dst, size_t dst_bytes);
int dsx_blosc_encode(const void* src, size_t bytes, int typesize, int clevel, int shuffle, void* frame,
                     size_t frame_capacity, size_t* frame_bytes);
/* The same with LZ4 inside (the host build of csrc/dsx_lz4_enc.h; no liblz4 needed): uint16 elements (bytes even),
 * byte shuffle, split streams -- the frames of DSX_ZENC_LZ4 below.  clevel 0 stores, 1 ... 9 encode alike. */
int dsx_io_write_chunks_blosc_lz4(dsx_ctx* ctx, const char* const* paths, const void* const* src,
                                  const size_t* bytes, int n, int threads, int clevel);
int dsx_blosc_encode_lz4(const void* src, size_t bytes, int clevel, void* frame, size_t frame_capacity,
                         size_t* frame_bytes);

/* Blosc-zstd frames of n_chunks uint16 chunks of chunk_bytes each, encoded on the device (csrc/dsx_zstd_enc.h:
 * entropy-only zstd -- Huffman literals, no matches -- in the container dsx_blosc_encode writes: 256 KiB blocks,
 * byte shuffle, "don't split"; a chunk that does not get smaller is a memcpyed frame).  d_src: the chunks back to
 * back (device); d_frames: the frames packed back to back, capacity n_chunks * (chunk_bytes + 16); d_offsets:
 * n_chunks + 1 int64 -- frame i is bytes [d_offsets[i], d_offsets[i + 1]).  typesize must be 2, chunk_bytes even;
 * clevel 0 stores every chunk, 1 ... 9 encode (the level does not change the encoding).  Asynchronous on the context
 * stream; the context keeps a work buffer of ~chunk_bytes + 64 per chunk.
 * dsx_blosc_encode_ref: the host build of the same encoder, byte-identical output (host pointers, synchronous).
 * The _ex forms take a mode.  DSX_ZENC_LITERALS: the above, byte for byte.  DSX_ZENC_RUNS: a zstd block may carry
 * sequences -- every run of >= 8 equal bytes inside a 128 KiB zstd block is one literal and one match of offset 1
 * (predefined FSE tables; at most 1024 sequences per block), the literals left are RLE, raw or Huffman; per zstd block
 * the smaller of the two encodings is written, so a frame is never larger than in DSX_ZENC_LITERALS.  On synthetic
 * (64, 128, 128) bricks: 1.00x the bytes of the host writer (zstd level 5) instead of 1.10x
 * (profiles/device_codec_runs_sizes.json).  No general matches, no offsets other than 1, typesize 2 only.  The
 * context keeps a second work buffer of the same size in this mode.
 * DSX_ZENC_LZ4: Blosc-LZ4 frames instead (csrc/dsx_lz4_enc.h: what c-blosc calls LZ4 with byte shuffle -- flags
 * SHUFFLE | 1 << 5, "don't split" clear: a full 256 KiB block is two LZ4 blocks, the low-byte and the high-byte plane,
 * each coded or stored on its own; a hash-table match finder, offsets 1 ... 65535), the frames dsx_blosc_encode_lz4
 * and dsx_io_write_chunks_blosc_lz4 write, byte for byte.  Any other mode: DSX_EINVAL. */
#define DSX_ZENC_LITERALS 0
#define DSX_ZENC_RUNS 1
#define DSX_ZENC_LZ4 3
int dsx_blosc_encode_device(dsx_ctx* ctx, const void* d_src, int n_chunks, size_t chunk_bytes, int typesize,
                            int clevel, void* d_frames, int64_t* d_offsets);
int dsx_blosc_encode_ref(const void* src, int n_chunks, size_t chunk_bytes, int typesize, int clevel, void* frames,
                         int64_t* offsets);
int dsx_blosc_encode_device_ex(dsx_ctx* ctx, const void* d_src, int n_chunks, size_t chunk_bytes, int typesize,
                               int clevel, void* d_frames, int64_t* d_offsets, int mode);
int dsx_blosc_encode_ref_ex(const void* src, int n_chunks, size_t chunk_bytes, int typesize, int clevel, void* frames,
                            int64_t* offsets, int mode);

/* Blosc chunks decoded on the device (csrc/dsx_zdec_task.h: the tasks; csrc/dsx_zdec_kernels.h: the kernels).
 * dsx_io_read_frames: n chunk files -> their frames packed back to back into `packed` (host memory, capacity
 * n * (chunk_bytes + 16)) and one 32-byte task per Blosc block into `tasks` (capacity n * (chunk_bytes / 8192 + 1)):
 * {uint64 src, uint64 dst, uint32 src_len, uint32 dst_len, uint32 kind, uint32 chunk}; chunk i decodes to bytes
 * [i * chunk_bytes, (i + 1) * chunk_bytes) of the output.  The device takes frames of typesize 2, no or byte shuffle,
 * zstd inside, unsplit streams, at most chunk_bytes / 8192 + 1 Blosc blocks (a zstd frame or a stored stream per
 * block), memcpyed frames and missing files (fill); any other frame is decoded on the I/O threads (dsx_blosc_decode)
 * and shipped as a copy.  routes (optional, n bytes): 0 device, 1 host, 2 fill.  Synchronous, no GPU involved (ctx may
 * be NULL).
 * dsx_blosc_decode_device: the tasks into d_out (out_bytes), asynchronous on the context stream; d_status receives
 * one int32 per task (0, or a dsx_zstd_dec.h Status for a malformed frame).  The context keeps a work buffer of
 * out_bytes.
 * dsx_blosc_decode_ref: the host build of the same decoder, byte-identical output (host pointers, synchronous).
 * dsx_io_read_frames_ex takes a mode.  DSX_ZDEC_ZSTD: the routes above, byte for byte.  DSX_ZDEC_ANY: the device also
 * takes (csrc/dsx_lz4_dec.h), still for typesize 2 and at most chunk_bytes / 8192 + 1 Blosc blocks:
 *     inner codec    zstd (no checksum), lz4, lz4hc            -> device     blosclz, zlib, snappy -> host
 *     shuffle        none, byte shuffle, bit shuffle           -> device
 *     block streams  unsplit, or split into 2 (low / high bytes; each stored or coded) -> device
 *     typesize != 2, zstd checksums, blocks under 8 KiB        -> host
 * `kind` of a task: 0 fill, 1 copy, 2 stored, 3 zstd, 4 lz4; | 0x100 byte un-shuffle, | 0x200 split (src is the int32
 * length word of the first of two streams, src_len spans both), | 0x400 bit un-shuffle.  One task per Blosc block in
 * either mode.  dsx_blosc_decode_device / _ref run the tasks of every mode.
 * DSX_ZDEC_ALL: DSX_ZDEC_ANY plus the last two inner codecs c-blosc 1.21 writes (csrc/dsx_inflate.h), in the same
 * layouts and under the same limits:
 *     inner codec    zstd (no checksum), lz4, lz4hc, blosclz, zlib -> device  snappy -> host
 * `kind` 5: one zlib stream (RFC 1950, its Adler-32 verified), 6: one blosclz stream; both take the 0x100 / 0x200 /
 * 0x400 bits.  Modes 0 and 1 route as before, byte for byte.  Any other mode, 2 included as before: DSX_EINVAL.
 * dsx_io_read_zlib_chunks: the chunk files of a store whose compressor is plain zlib (the whole file is one zlib
 * stream) packed like frames: one task of kind 5 per chunk with dst_len = chunk_bytes and no shuffle (capacities:
 * n * (chunk_bytes + 16) bytes, n tasks); a missing file is a fill task; a file longer than chunk_bytes + 16 is
 * inflated on the I/O threads and shipped as a copy (route 1). */
#define DSX_ZDEC_ZSTD 0
#define DSX_ZDEC_ANY 1
#define DSX_ZDEC_ALL 3
int dsx_io_read_frames_ex(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                          uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                          size_t* packed_bytes, int* n_tasks, uint8_t* routes, int mode);
int dsx_io_read_frames(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                       uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                       size_t* packed_bytes, int* n_tasks, uint8_t* routes);
int dsx_io_read_zlib_chunks(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                            uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                            size_t* packed_bytes, int* n_tasks, uint8_t* routes);
int dsx_blosc_decode_device(dsx_ctx* ctx, const void* d_packed, size_t packed_bytes, const void* d_tasks, int n_tasks,
                            void* d_out, size_t out_bytes, int32_t* d_status);
int dsx_blosc_decode_ref(const void* packed, size_t packed_bytes, const void* tasks, int n_tasks, void* out,
                         size_t out_bytes, int32_t* status);

/* PNG scanline reconstruction for the directory mode's reader (imageio's iio.imread, readers.py:86-87): `height`
 * rows of one filter-type byte + `stride` bytes, un-filtered in place (Sub / Up / Average / Paeth).  Host only.  */
int dsx_png_unfilter(void* rows, int height, int stride, int bytes_per_pixel);

/* flatfield_correction() of one plane as a stand-alone call (filtering.py:338-414): dark subtraction
 * (integer planes truncate, :400-403), division by the flat, baseline, clip, uint16.  dark is
 * [dark_h][dark_w] >= the plane and is cropped to it (:377).  Device pointers, asynchronous.   */
/* Stack mode = the 3-D input mode of log_space_fft_filtering() (filtering.py:182-183, 188, 210-211): the planes of
 * ONE dsx_run_* call are a stack that shares one Otsu threshold per decomposition level (min / max of cH^2 and the
 * 256-bin histogram are taken over all planes; row medians and the FFT stay per plane row).  The whole stack must
 * fit one cohort (n <= max_batch of dsx_plan, else DSX_ELIMIT).  Off by default: planes are independent.       */
int dsx_set_stack_mode(dsx_ctx* ctx, int on);

int dsx_flatfield_correction(dsx_ctx* ctx, const void* d_img, int in_dtype, int H, int W,
                             const float* d_flat, const float* d_dark, int dark_h, int dark_w,
                             float baseline, void* d_out);
/* The same with one baseline value per plane ROW (d_baseline_rows: H floats on the device, NULL = the scalar): what
 * the reference's broadcast baseline[:, np.newaxis] does for a 2-D plane and a baseline of length H
 * (filtering.py:393-398, 409).                                                                              */
int dsx_flatfield_correction_rows(dsx_ctx* ctx, const void* d_img, int in_dtype, int H, int W,
                                  const float* d_flat, const float* d_dark, int dark_h, int dark_w,
                                  float baseline, const float* d_baseline_rows, void* d_out);

/* get_foreground_background_mean() as a stand-alone call (filtering.py:54-88): a pixel is foreground
 * when float16(pixel) >= cutoff (the host derives cutoff from threshold_mask, 383.25 for the default
 * 0.3); means in double, 0.0 for an empty class; d_mask (nullable) gets 1 / 0 per pixel.
 * Synchronous.  Inside dsx_run_* the same statistic is fused into the first analysis kernel.      */
int dsx_foreground_background(dsx_ctx* ctx, const void* d_img, int in_dtype, size_t n, float cutoff,
                              double* fore_mean, double* back_mean, void* d_mask);

/* ---- multi-GPU: one process per GPU, z-ranges per rank, ONE collective ---- */
/* The reference parallelises over chunks with OS processes and a queue (zarr_destriper.py:1138-1172)
 * and never communicates between workers; planes are independent (:319-327).  Here the only exchange
 * is a broadcast (root 0) of the constant blob / shading planes before the data path, straight on
 * RCCL over xGMI (librccl.so is dlopen'ed by the first dsx_comm_* call; no torch).  Rank 0 creates
 * the 128-byte unique id and hands it to the other ranks through any host channel (file, env,
 * socket: aind_smartspim_destripe_amd/distributed.py has a file rendezvous), then every rank calls
 * dsx_comm_init -- which is collective.  Broadcast / all-reduce run on the context stream and are
 * synchronous; an all-reduce doubles as a barrier.                                               */
#define DSX_COMM_ID_BYTES 128
int dsx_comm_unique_id(dsx_ctx* ctx, char* id, size_t id_bytes);
int dsx_comm_init(dsx_ctx* ctx, const char* id, size_t id_bytes, int rank, int world);
int dsx_comm_destroy(dsx_ctx* ctx);
/* In place on device memory: root's bytes replace everybody else's. */
int dsx_comm_broadcast(dsx_ctx* ctx, void* d_buf, size_t bytes, int root);
/* Host doubles (n <= 64) reduced over the ranks: op 0 = sum, 1 = max, 2 = min. */
int dsx_comm_allreduce_f64(dsx_ctx* ctx, double* values, int n, int op);

/* ---- dual-band wavelet-FFT stripe filter (filter_streaks with sigma = (fg, bg)) -------------- */
/* The upstream pystripe filter built from the reference's helpers (foreground_fraction, gaussian_filter,
 * filtering.py:25-51, 91-136): per plane a threshold t (skimage threshold_otsu of the input, or fixed), the
 * edge-padded even plane split into min(x, t) and max(x, t), each band log(1 + z) -> wavedec2 (mode symmetric) ->
 * every cH row irfft(rfft(cH) * notch(s)), s = h_l * sigma / H' -> waverec2 -> exp(r) - 1, then
 * out = f * w + b * (1 - w), w = sigmoid((x - t) / crossover), cropped to [H, W].  sigma_fg == sigma_bg runs ONE
 * band on the unclipped plane.  A streaks plan replaces any plan of the context (dsx_plan replaces it in turn);
 * dsx_run_host / dsx_run_device then run it: [n, H, W] in, [n, H, W] out (uint16: clip + truncate).          */
typedef struct dsx_streaks_cfg {
  int32_t wavelet;    /* DSX_WAVELET_DB3, or DSX_WAVELET_BANK (the bank of the last dsx_set_wavelet)        */
  int32_t level;      /* 0 == maximum level (pywt.dwt_max_level(min(H', W'), filter length)), else the depth */
  float sigma_fg;     /* > 0                                                                               */
  float sigma_bg;     /* > 0                                                                               */
  float crossover;    /* > 0                                                                               */
  int32_t otsu;       /* 1: t = threshold_otsu of each plane; 0: t = threshold                             */
  float threshold;
} dsx_streaks_cfg;
int dsx_plan_streaks(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_streaks_cfg* cfg);
/* The same plan with a choice of kernels.  DSX_STREAKS_GENERIC: dsx_plan_streaks, byte for byte.  DSX_STREAKS_MARCH:
 * the bands run through the marching db3 kernels and the FFT row filter of the log-space engine.  With an empty mask
 * log_space_fft_filtering(z, sigma = s min(H, W) / H) - 2 IS band(z, s), so per cohort: t as above (same kernels,
 * same t), then one kernel writes the bands max(x, t) / min(x, t) as virtual input planes 2k / 2k + 1 (uint16 where the
 * planes are uint16 and t is integral, else float32; one plane per real plane for equal sigmas), the log-space chain
 * of dsx_plan runs over them with cfg = plane index & 1 and every level's mask threshold +inf (no histogram, no Otsu
 * per level), and one kernel blends (F - 2) w + (B - 2) (1 - w), crops and stores.  For DSX_WAVELET_DB3, even
 * height and width, a level up to the maximum level, and every geometry dsx_plan accepts; anything else: DSX_EINVAL (DSX_ELIMIT where dsx_plan
 * says so).  Any other route: DSX_EINVAL. */
#define DSX_STREAKS_GENERIC 0
#define DSX_STREAKS_MARCH 1
int dsx_plan_streaks_ex(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_streaks_cfg* cfg, int route);
/* Options of the blend (the three upstream pystripe forms the plain plan leaves out).  All zero == no option.
 *   bands      DSX_STREAKS_BANDS_BOTH: out = f w + b (1 - w).  _FG: only the foreground band is filtered,
 *              out = f w + x (1 - w); _BG: only the background band, out = x w + b (1 - w).  A one-sided plan runs ONE
 *              band through the whole chain and does not read the other sigma of the cfg.
 *   smoothing  0: w = sigmoid((x - t) / crossover) on the unpadded [H, W] plane.  0 < s <= 2:
 *              w = scipy.ndimage.gaussian_filter(sigmoid, s) with that function's defaults (separable, radius
 *              int(4 s + 0.5), taps exp(-k^2 / 2 s^2) normalised to sum 1, half-sample reflection at the border).
 *              Anything else (negative, above 2, not finite): DSX_EINVAL.  Equal sigmas have no w: accepted, no effect.
 *   flat/dark  host float32 planes, NULL together: flat [H, W], dark [dark_h, dark_w] with dark_h >= H and
 *              dark_w >= W (cropped by indexing).  The float result r goes through flatfield_correction(r, flat, dark):
 *              r > dark ? r - dark : 0, / flat, clip to [0, 65535]; uint16 output truncates, float32 output is the
 *              clipped value.
 * With any option set, one tiled kernel (k_st_blendx, dsx_streaks.h) does the blend on either route; with none,
 * dsx_plan_streaks_opts IS dsx_plan_streaks_ex, byte for byte and launch for launch. */
#define DSX_STREAKS_BANDS_BOTH 0
#define DSX_STREAKS_BANDS_FG 1
#define DSX_STREAKS_BANDS_BG 2
typedef struct dsx_streaks_opts {
  int32_t bands;      /* DSX_STREAKS_BANDS_*                                                                */
  float smoothing;    /* 0, or 0 < s <= 2                                                                   */
  const float* flat;  /* host, [H, W], or NULL                                                              */
  const float* dark;  /* host, [dark_h, dark_w], NULL exactly when flat is                                  */
  int32_t dark_h;
  int32_t dark_w;
} dsx_streaks_opts;
/* opts NULL or all zero: dsx_plan_streaks_ex. */
int dsx_plan_streaks_opts(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_streaks_cfg* cfg, int route,
                          const dsx_streaks_opts* opts);
/* Host build of the options blend over ONE plane, compiled from the same weight, fold, tap, blend and epilogue
 * functions as the kernel: x, f, b float32 [H, W] (the plane and the band values f = band(max(x, t), sigma_fg),
 * b = band(min(x, t), sigma_bg); the band a one-sided opts->bands does not read may be NULL), t, crossover and opts
 * as above (flat / dark host planes); out [H, W] of out_dtype.  No context and no device call; the message of an
 * error is read with dsx_last_error(NULL). */
int dsx_streaks_blend_ref(const float* x, const float* f, const float* b, int height, int width, float t,
                          float crossover, const dsx_streaks_opts* opts, void* out, int out_dtype);
/* t of a plane of the last cohort of the last run (a bin centre for float32 planes, an integer for uint16). */
int dsx_get_streaks_threshold(dsx_ctx* ctx, int plane, float* threshold);

/* ---- light-sheet background mode (csrc/dsx_lightsheet.h; DESIGN.md "Light-sheet background mode") -----------------
 * Per uint16 plane x[height, width], stripes along x:
 *   q      = number of edges[v] <= x        (edges: 255 non-decreasing values, edges[v - 1] = smallest x with q >= v)
 *   P(h,w) = the windowed percentile of scikit-image's rank.percentile(q, ones((h, w)), p0 = p): rows i - h/2 ..
 *            i - h/2 + h - 1, columns j - w/2 .. j - w/2 + w - 1, only the n pixels inside the plane counted, the
 *            smallest v with #{q <= v} >= floor(p n) + 1 (p n in float64)
 *   L = back[P(1, A)], G = back[P(B, B)];  offset = L <= (float)lambda * G ? L : G;  out = max((float)x - offset, 0)
 * 0 < p < 1, 1 <= A <= 1024, 1 <= B <= 255, lambda > 0; edges and back (256 float32) are host tables and are copied.
 * The plan replaces any other and serves dsx_run_host / dsx_run_device: uint16 in, uint16 (truncated) or float32 out,
 * anything else DSX_EINVAL; cfg_used is not written.  It honours dsx_set_rotate. */
int dsx_plan_lightsheet(dsx_ctx* ctx, int height, int width, int max_batch, double p, int A, int B, double lambda,
                        const uint32_t* edges, const float* back);
/* The host build of the same arithmetic over ONE plane (host pointers, no context, no device call): out [H, W] of
 * out_dtype; ls and bg (uint8 [H, W], the two percentile planes) may be NULL.  dsx_last_error(NULL) has the message. */
int dsx_lightsheet_ref(const void* x, int height, int width, double p, int A, int B, double lambda,
                       const uint32_t* edges, const float* back, uint8_t* ls, uint8_t* bg, void* out, int out_dtype);
/* Debug hook: the ls and bg planes (uint8 [h, w] each, of the plan's own -- with dsx_set_rotate the rotated --
 * orientation; either may be NULL) of plane `plane` of the last cohort of the last run.  Synchronises. */
int dsx_get_lightsheet_planes(dsx_ctx* ctx, int plane, uint8_t* ls, uint8_t* bg);

/* ---- parity / debug hooks (state of the LAST cohort of the last run) ----------------------- */
/* Per plane of the last cohort: fore/back means and chosen config (filtering.py:459-462). */
int dsx_get_stats(dsx_ctx* ctx, int plane, double* fore_mean, double* back_mean,
                  int32_t* cfg_used);
/* Per plane and level (0 == finest): Otsu value (of cH^2) and the threshold actually used. */
int dsx_get_thresholds(dsx_ctx* ctx, int plane, int level, float* otsu, float* threshold);
/* Copy a level buffer [h, w] (float32, dense) of a plane to the host. */
int dsx_get_level(dsx_ctx* ctx, int plane, int level, int stage, float* out);
/* Stop the pipeline after a stage (0 == run everything, 1 == after the forward transform +
 * thresholds, 2 == after the row filter) so that dsx_get_level can read cH / Delta.           */
int dsx_set_stop_after(dsx_ctx* ctx, int stage);

#ifdef __cplusplus
}
#endif
#endif /* DSX_H */
