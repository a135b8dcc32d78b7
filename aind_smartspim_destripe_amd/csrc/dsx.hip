// dsx.hip -- C ABI of the MI355X destripe engine (see include/dsx.h) and the launch pipeline.
//
// Pipeline per cohort part (a cohort of <= max_batch planes is split into parts that run on separate
// HIP streams; no host synchronisation inside) -- run_cohort and its stages; what is fused and every grid, block and
// LDS size is decided by dsx_chain.h:
//   k_zero3  ->  k_fwd_march<fused: levels 1 + 2>, k_fwd_march per level from 3  ->  k_hist (one launch per stream)
//   ->  k_otsu  ->  k_rowfilter (level 2), k_rowfilter_pack (the coarse levels in one launch, several row pairs per
//       wave; DSX_NO_ROW_PACK=1: k_rowfilter_multi, one pair per wave)
//   ->  k_inv_march per level down to 3  ->  k_rowfinal (level-1 row filter + levels 2 and 1 of the synthesis + finish)
// An unsplit cohort runs the wide levels' k_hist and k_rowfilter on a helper stream beside the coarse levels' launches.
// Planes the fused kernels do not take (widths that are no multiple of 4 / 8, float32, other FFT plans) fall back piece
// by piece: k_inv_march<fused final> + k_rowfilter for level 1, one k_fwd_march / k_inv_march per level.
// A wavelet other than db3 (dsx_set_wavelet) swaps k_fwd_gen / k_inv_gen (dsx_wavelet.h) in for the marching kernels.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is dlopen'ed by dsx_comm_init
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dsx.h"
#include "dsx_kernels.h"
#include "dsx_retile.h"
#include "dsx_rot90.h"
#include "dsx_pyramid.h"
#include "dsx_stackrank.h"
#include "dsx_smooth.h"
#include "dsx_volhist.h"
#include "dsx_project.h"
#include "dsx_digest.h"
#include "dsx_wavelet.h"
#include "dsx_plan.h"
#include "dsx_chain.h"
#include "dsx_io.h"
#include "dsx_streaks.h"
#include "dsx_lightsheet.h"
#include "dsx_zenc_kernels.h"
#include "dsx_lz4enc_kernels.h"
#include "dsx_zdec_kernels.h"

namespace {

thread_local std::string g_init_error;

enum KernelClass { KC_FWD1 = 0, KC_FWD, KC_HIST, KC_OTSU, KC_ROW, KC_INV, KC_FINAL, KC_COUNT };
const char* kClassNames[KC_COUNT] = {"k_fwd_march(level1)", "k_fwd_march(coarse)", "k_hist", "k_otsu",
                                     "k_rowfilter",       "k_inv_march(pyramid)", "k_inv_march(final)"};

struct ProfRec {
  int cls;
  hipEvent_t e0, e1;
};

}  // namespace

struct dsx_ctx {
  int device = 0;
  DsxTuning tune;
  int cus = 256;  // compute units of the device (march_segments' launch-quantisation score); 256 when it does not say
  hipStream_t stream_ = nullptr;  // the context ("compute") stream; entry points reach it through use_main()
  std::string err;
  bool planned = false;
  dsx::Plan plan;
  dsx::HostCfg cfg[2];
  double high_int = 2700.0;
  int max_batch = 0;
  // sigmoid(float16((x - 400) / 20)) > 0.3 of filtering.py:78-80  <=>  float16(x) >= 383.25  <=>
  // x > 383.125 (round-to-nearest-even), checked against every float16 pattern in tests/golden
  float fg_cutoff = 383.12503f;
  // device buffers
  float* d_ws = nullptr;          // [max_batch][plane_floats]
  char* d_ctl = nullptr;          // control block, zeroed per cohort (stats | minmax | hist)
  size_t ctl_zero_bytes = 0;
  dsx::PlaneStats* d_stats = nullptr;
  unsigned* d_minmax = nullptr;
  unsigned* d_hist = nullptr;
  float* d_thr = nullptr;
  float* d_otsu = nullptr;
  int* d_cfg = nullptr;
  double* d_means = nullptr;
  dsx::C32* d_consts = nullptr;
  size_t consts_bytes = 0;
  float* d_flat = nullptr;
  float* d_dark = nullptr;
  bool own_shading = false;
  int dark_h = 0, dark_w = 0;
  // staging for dsx_run_host
  void* d_stage_in = nullptr;
  void* d_stage_out = nullptr;
  size_t stage_in_bytes = 0, stage_out_bytes = 0;
  // last cohort (debug hooks)
  int last_n = 0;
  int stop_after = 0;
  // timing
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool profiling = false;
  std::vector<ProfRec> prof;
  size_t workspace_bytes = 0;
  // filter bank given by dsx_set_wavelet (wl_len == 0: db3, the specialised marching kernels)
  int wl_len = 0;          // bank in use by the current plan
  int wl_bank_len = 0;     // bank given by the last dsx_set_wavelet
  bool wl_set = false;
  float wl[4][dsx::kMaxTaps] = {};       // dec_lo, dec_hi, rec_lo, rec_hi of the current plan
  float wl_bank[4][dsx::kMaxTaps] = {};  // ... of the last dsx_set_wavelet
  // Sticky flag word in pinned host memory, written by k_otsu when a plane's PlaneStats::flags is set (a float32
  // pixel whose log(1 + x) is not finite).  The asynchronous device-buffer path (dsx_run_device) cannot raise at
  // the call; the next synchronising entry point (dsx_sync, dsx_event_sync, dsx_stream_sync, dsx_get_stats) reports
  // DSX_EVALUE instead and clears the word.
  unsigned* h_sticky = nullptr;
  // dsx_blosc_encode_device: encoded zstd blocks (slots) and their sizes, grown on demand (grow_device; *_bytes held)
  uint8_t* zenc_slots = nullptr;
  uint32_t* zenc_sizes = nullptr;
  size_t zenc_slot_bytes = 0, zenc_size_bytes = 0;
  uint8_t* zenc_lits = nullptr;  // runs mode: the literals the runs leave, per zstd block
  size_t zenc_lit_bytes = 0;
  // dsx_blosc_decode_device: shuffled blocks are decoded here before the un-shuffle, grown on demand
  uint8_t* zdec_scratch = nullptr;
  size_t zdec_bytes = 0;
  unsigned* d_sticky = nullptr;
  // dsx_volhist_*: 65 536 uint64 bins, allocated by the first dsx_volhist_reset; no plan call touches it
  unsigned long long* volhist = nullptr;
  // dsx_set_stack_mode: the planes of a call share ONE Otsu threshold per level (the reference's 3-D input mode)
  bool stack_mode = false;
  // DSX_ABLATE environment variable (timing-only switches that return WRONG pixels): read only by a library built
  // with -DDSX_DIAG (tools/build_variant.sh); the product build has no such switch
  int ablate = 0;
  // sub-cohort streams: a cohort is split into parts that run their launch chains concurrently, so that
  // latency-bound (march) and compute-bound (row filter) kernels of different parts overlap on the chip
  static constexpr int kMaxStreams = 8;
  int n_streams = 4;
  hipStream_t aux[kMaxStreams] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams] = {};
  // Cross-call pipelining of the sub-cohort streams: the joins of a split cohort are deferred until something
  // else needs the context stream, so that an identical run_device call that follows (the next batch of a
  // steady stream of batches) starts each part right behind the same part of the call before it.
  // Helper stream per part: the wide levels' histogram / row filter run beside the coarse levels' launches
  // (small grids that leave most of the chip idle), see run_cohort
  hipStream_t helper[kMaxStreams] = {};
  hipEvent_t ev_h[kMaxStreams][4] = {};
  int joins_pending = 0;              // parts (incl. part 0) of a split cohort the context stream has not joined yet
  unsigned long long main_ops = 0;    // operations entry points put on the context stream (use_main calls)
  struct {
    const void* in = nullptr; void* out = nullptr; const void* cfg = nullptr;
    int n = 0, in_dtype = 0, out_dtype = 0, parts = 0;
    unsigned long long main_ops = 0;
  } last_split;
  // multi-GPU: RCCL communicator of the one collective of the path (dsx_comm_*)
  void* rccl = nullptr;  // dlopen handle of librccl.so
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  double* d_red = nullptr;  // scratch of dsx_comm_allreduce_f64
  // copy streams of the overlapped chunk map (dsx_memcpy_*_async): 1 = upload, 2 = download
  hipStream_t copy_stream[2] = {};
  hipEvent_t ev_xs = nullptr;  // cross-stream ordering (dsx_stream_wait)
  static constexpr int kEventSlots = 8;
  hipEvent_t ev_slot[kEventSlots] = {};  // host-visible completion marks (dsx_event_record / dsx_event_sync)
  // HIP graphs of unsplit cohorts (run_cohort_split), OPT-IN with DSX_GRAPH=1: the launch chain of a (planes, result,
  // count, types) tuple is captured the second time the tuple is seen and replayed from then on -- one graph launch
  // instead of ~30 kernel launches and 4 cross-stream events for the per-slice calls of the reference's API
  // (filter_stripes: 1 plane).  Measured on ROCm 7.2 / MI355X (tools/latency_small.py, profiles/r2_latency_small.txt):
  // bit-identical results, but 5-8 % SLOWER than the eager launches (1 plane of 2048^2: 515 against 473 us per call,
  // the enqueue takes 130 us either way), so eager stays the default.
  struct GraphEntry {
    const void* in; void* out; const void* cfg;
    int n, in_dtype, out_dtype, seen;
    hipGraphExec_t exec;
    unsigned long long last_use;
  };
  static constexpr int kGraphSlots = 8;
  std::vector<GraphEntry> graphs;
  unsigned long long graph_clock = 0;
  int graph_mode = 0;  // DSX_GRAPH=1 turns graphs on; back to 0 when a capture fails on this runtime
  unsigned long long graph_launches = 0, graph_captures = 0;
  unsigned long long row_pack_launches = 0;  // k_rowfilter_pack launches enqueued (dsx_row_pack_launches)
  // dual-band filter (dsx_plan_streaks): when set, dsx_run_* run this plan instead of the log-space one
  bool streaks = false;
  dsx::st::StreaksPlan sp;
  float* st_ws = nullptr;         // [regions of sp][P virtual planes]
  float* st_mat = nullptr;        // row-filter operators, sp.lv[l].mat_off[band]
  unsigned* st_mm = nullptr;      // [max_batch][2] min / max keys
  unsigned* st_hist = nullptr;    // [max_batch][kStBins]
  float* st_t = nullptr;          // [max_batch] threshold per plane
  dsx::st::OtsuOut* st_info = nullptr;
  // march route of the streaks plan (DSX_STREAKS_MARCH): `plan` holds the log-space chain over the virtual band planes
  // (cfg 0 / 1 = foreground / background band), run_cohort launches neither k_hist nor k_otsu
  bool st_march = false;
  int st_vdtype = DSX_U16;        // element type of the virtual planes of uint16 input (float32 input: float32)
  void* st_vin = nullptr;         // [bands * B][H][W] virtual input planes
  float* st_vout = nullptr;       // [bands * B][H][W] what the chain writes: band + 2
  // options of the blend (dsx_plan_streaks_opts); st_opts false: k_st_final / k_st_blend, as dsx_plan_streaks_ex
  bool st_opts = false;
  int st_mode = dsx::st::kStBoth; // kStBoth / kStFg / kStBg / kStSingle
  int st_R = 0;                   // radius of the weight smoothing, 0: none
  float st_taps[dsx::st::kStMaxR + 1] = {};
  float* st_flat = nullptr;       // [H][W], or nullptr: no dark / flat step
  float* st_dark = nullptr;       // [>= H][st_dark_w]
  int st_dark_w = 0;
  // dsx_set_rotate: the next plan is made for np.rot90 of the caller's planes.  `rot`: the current plan is such a plan
  // -- its chain (or streaks plan) holds the rotated geometry, rot_H x rot_W is the caller's plane, and the run entry
  // points turn every plane into rot_in ahead of the chain and its result out of rot_out behind it (dsx_rot90.h).  The
  // two buffers hold max_batch planes and are sized by the element types of the first run that needs them.
  bool rot_next = false;
  bool rot = false;
  int rot_H = 0, rot_W = 0;
  void* rot_in = nullptr;
  void* rot_out = nullptr;
  size_t rot_in_bytes = 0, rot_out_bytes = 0;
  // light-sheet background mode (dsx_plan_lightsheet): when set, dsx_run_* run this plan.  ls_H x ls_W is the plane the
  // kernels see (the rotated one of a rotated plan); ls_q / ls_ls / ls_bg hold max_batch uint8 planes each
  bool lightsheet = false;
  int ls_H = 0, ls_W = 0, ls_A = 0, ls_B = 0;
  double ls_p = 0.0;
  float ls_lambda = 0.f;
  uint32_t* ls_edges = nullptr;   // [kLsEdges]
  float* ls_back = nullptr;       // [256]
  uint8_t* ls_q = nullptr;
  uint8_t* ls_ls = nullptr;
  uint8_t* ls_bg = nullptr;
};

namespace {
// Buffers of one part of a cohort (planes [po, po + nb) of the workspace) and the stream it runs on.
struct CohortView {
  hipStream_t stream;
  hipStream_t helper;   // nullptr: everything on `stream`
  hipEvent_t* ev;       // 4 events of this part (helper fork / join, twice)
  bool alone;           // the cohort runs as ONE part: its big kernels have the chip to themselves (march_segments)
  float* ws;
  dsx::PlaneStats* stats;
  unsigned* minmax;
  unsigned* hist;
  float* thr;
  float* otsu;
  int* cfg;
  double* means;
};
}  // namespace

namespace {

int fail(dsx_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_init_error = msg;  // context-free calls (dsx_io_*): dsx_last_error(NULL) reports it
  return code;
}

// The context stream for an entry point: first waits for the sub-cohort streams of a split cohort that is
// still running (deferred joins), and notes that the stream has been used.
hipStream_t use_main(dsx_ctx* c) {
  for (int i = 1; i < c->joins_pending; ++i) (void)hipStreamWaitEvent(c->stream_, c->ev_join[i], 0);
  c->joins_pending = 0;
  ++c->main_ops;
  return c->stream_;
}

#define DSX_HIP(call)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(ctx, DSX_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
  } while (0)

void drop_graphs(dsx_ctx* c) {
  for (auto& g : c->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  c->graphs.clear();
}

void free_plan_buffers(dsx_ctx* c) {
  drop_graphs(c);  // they hold the addresses of the buffers freed below
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(c->d_ws); c->d_ws = nullptr;
  fr(c->d_ctl); c->d_ctl = nullptr;
  fr(c->d_thr); c->d_thr = nullptr;
  fr(c->d_otsu); c->d_otsu = nullptr;
  fr(c->d_cfg); c->d_cfg = nullptr;
  fr(c->d_means); c->d_means = nullptr;
  fr(c->d_consts); c->d_consts = nullptr;
  if (c->own_shading) { fr(c->d_flat); fr(c->d_dark); }
  c->d_flat = c->d_dark = nullptr;
  c->own_shading = false;
  fr(c->d_stage_in); c->d_stage_in = nullptr; c->stage_in_bytes = 0;
  fr(c->d_stage_out); c->d_stage_out = nullptr; c->stage_out_bytes = 0;
  fr(c->rot_in); c->rot_in = nullptr; c->rot_in_bytes = 0;
  fr(c->rot_out); c->rot_out = nullptr; c->rot_out_bytes = 0;
  c->rot = false;
  c->planned = false;
}

struct LaunchScope {
  dsx_ctx* c;
  bool on;
  ProfRec r;
  LaunchScope(dsx_ctx* c_, int cls) : c(c_), on(c_->profiling) {
    if (on) {
      r.cls = cls;
      (void)hipEventCreate(&r.e0);
      (void)hipEventCreate(&r.e1);
      (void)hipEventRecord(r.e0, c->stream_);
    }
  }
  ~LaunchScope() {
    if (on) {
      (void)hipEventRecord(r.e1, c->stream_);
      c->prof.push_back(r);
    }
  }
};

// Raises a kernel's dynamic LDS limit, once per device (one flag array per kernel: a template over its address).
template <auto KERN>
hipError_t raise_lds_limit(size_t bytes = dsx::kLdsLimit) {
  static bool done[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (done[dev & 63]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done[dev & 63] = true;
  return e;
}

template <int CPL, int GF = -1, int NT = -1, int HALO = -1, int PLAN = 0>
hipError_t launch_rowfilter(const DsxTuning& t, const dsx::RowArgs& a, int npairs, int nb, hipStream_t s) {
  if (hipError_t e = raise_lds_limit<dsx::k_rowfilter<CPL, GF, NT, HALO, PLAN>>()) return e;
  const dsx::RowLaunch g = dsx::rowfilter_launch(t, CPL, a.M, npairs);
  hipLaunchKernelGGL((dsx::k_rowfilter<CPL, GF, NT, HALO, PLAN>), dim3(g.grid_x, nb), dim3(64 * g.wpb), g.lds, s, a);
  return hipGetLastError();
}

// rows longer than one wave holds: one 512-lane block per row pair, the row buffer is the block's LDS
hipError_t launch_rowfilter_wide(const dsx::RowArgs& a, int npairs, int nb, hipStream_t s) {
  if (hipError_t e = raise_lds_limit<dsx::k_rowfilter_wide>(dsx::kWideMaxLen * sizeof(float2))) return e;
  if (a.M > dsx::kWideMaxLen || a.w >= 65536) return hipErrorInvalidValue;  // (the plan refuses these lengths)
  hipLaunchKernelGGL(dsx::k_rowfilter_wide, dim3(npairs, nb), dim3(dsx::kWideThreads), (size_t)a.M * sizeof(float2), s, a);
  return hipGetLastError();
}

// the instantiation of a compile-time plan: its template arguments are its row of dsx::kRowPlans
template <int ID>
hipError_t launch_rowfilter_plan(const DsxTuning& t, const dsx::RowArgs& a, int npairs, int nb, hipStream_t s) {
  constexpr dsx::RowPlan p = dsx::row_plan(ID);
  return launch_rowfilter<p.cpl, p.gf, p.nt, p.halo, ID>(t, a, npairs, nb, s);
}

// the k_rowfilter instantiation of a row's class (dsx::classify_row)
// (the compiler emits the kernels in the order in which they are named here: keep it when a plan is added)
hipError_t dispatch_rowfilter(const DsxTuning& t, const dsx::RowArgs& a, int npairs, int nb, hipStream_t s) {
  const dsx::RowClass c = dsx::classify_row(a.M, a.w, a.K, a.npass, a.radix);
  if (c.wide) return launch_rowfilter_wide(a, npairs, nb, s);
  switch (c.cpl) {
    case 2: return launch_rowfilter<2>(t, a, npairs, nb, s);
    case 4: return launch_rowfilter<4>(t, a, npairs, nb, s);
    case 6: return launch_rowfilter<6>(t, a, npairs, nb, s);
    case 10: return launch_rowfilter<10>(t, a, npairs, nb, s);
    case 18:
      if (c.plan == 1) return launch_rowfilter_plan<1>(t, a, npairs, nb, s);
      if (c.gf == 4) return launch_rowfilter<18, 4, 1, 0>(t, a, npairs, nb, s);
      if (c.plan == 2) return launch_rowfilter_plan<2>(t, a, npairs, nb, s);
      if (c.gf == 2) return launch_rowfilter<18, 2, 1, 1>(t, a, npairs, nb, s);
      if (c.plan == 5) return launch_rowfilter_plan<5>(t, a, npairs, nb, s);
      if (c.plan == 6) return launch_rowfilter_plan<6>(t, a, npairs, nb, s);
      return launch_rowfilter<18>(t, a, npairs, nb, s);
    default:
      if (c.plan == 3) return launch_rowfilter_plan<3>(t, a, npairs, nb, s);
      if (c.plan == 4) return launch_rowfilter_plan<4>(t, a, npairs, nb, s);
      return launch_rowfilter<36>(t, a, npairs, nb, s);
  }
}

template <int ID>
hipError_t launch_rowfinal_plan(const dsx::RowFinalArgs& a, int nb, hipStream_t s) {
  constexpr dsx::RowPlan p = dsx::row_plan(ID);
  constexpr auto kernel = dsx::k_rowfinal<p.cpl, p.gf, p.nt, p.halo, ID>;
  if (hipError_t e = raise_lds_limit<kernel>()) return e;
  const dsx::RowLaunch g = dsx::rowfinal_launch(a.r.M, a.f.hout);
  hipLaunchKernelGGL(kernel, dim3(g.grid_x, nb), dim3(64 * g.wpb), g.lds, s, a);
  return hipGetLastError();
}

// plan: dsx::rowfinal_plan of the part (the plan id the classifier gives level 1)
hipError_t launch_rowfinal(int plan, const dsx::RowFinalArgs& a, int nb, hipStream_t s) {
  if (plan == 1) return launch_rowfinal_plan<1>(a, nb, s);
  if (plan == 3) return launch_rowfinal_plan<3>(a, nb, s);
  if (plan == 4) return launch_rowfinal_plan<4>(a, nb, s);
  return hipErrorInvalidValue;
}

// Levels whose row filters all fit the CPL = 6 class, in ONE launch (k_rowfilter_multi).
hipError_t launch_rowfilter_multi(const dsx::RowMultiArgs& a_in, const int* npairs, int nb, hipStream_t s) {
  if (hipError_t e = raise_lds_limit<dsx::k_rowfilter_multi<6>>()) return e;
  dsx::RowMultiArgs a = a_in;
  int M[dsx::kRowMultiMax];
  for (int i = 0; i < a.nlev; ++i) M[i] = a.lv[i].M;
  const dsx::RowLaunch g = dsx::row_multi_launch(a.nlev, npairs, M, a.blk_end);
  hipLaunchKernelGGL(dsx::k_rowfilter_multi<6>, dim3(g.grid_x, nb), dim3(64 * g.wpb), g.lds, s, a);
  return hipGetLastError();
}

// ... with several row pairs per wave (k_rowfilter_pack): pack factor per level and geometry from dsx_chain.h
hipError_t launch_rowfilter_pack(const DsxTuning& t, const dsx::RowMultiArgs& m, const int* npairs, int nb, hipStream_t s) {
  if (hipError_t e = raise_lds_limit<dsx::k_rowfilter_pack<6>>()) return e;
  dsx::RowPackArgs a;
  memset(&a, 0, sizeof(a));
  a.nlev = m.nlev;
  int M[dsx::kRowMultiMax];
  for (int i = 0; i < m.nlev; ++i) {
    a.lv[i] = m.lv[i];
    M[i] = m.lv[i].M;
    a.pack[i] = dsx::row_pack_factor(t, m.lv[i].M, m.lv[i].npass, m.lv[i].radix);
  }
  const dsx::RowLaunch g = dsx::row_pack_launch(t, a.nlev, npairs, M, a.pack, a.blk_end);
  hipLaunchKernelGGL(dsx::k_rowfilter_pack<6>, dim3(g.grid_x, nb), dim3(64 * g.wpb), g.lds, s, a);
  return hipGetLastError();
}

// One cohort part on its way through the chain: what the stages of run_cohort share.
struct Chain {
  dsx_ctx* ctx;
  const CohortView& v;
  dsx::ChainShape sh;
  const void* d_in;
  int in_dtype, nb;
  void* d_out;
  int out_dtype;
};

// DSX_SKIP_HIST / DSX_SKIP_ROW: bit masks of level indices whose histogram / row-filter launch is left out, and
// DSX_SKIP_COARSE=k: no launch for levels with index >= k (what the chain would gain if those kernels were free).
// The results are WRONG: the switches only exist in a -DDSX_DIAG build.
struct Skips {
  int hist, row, from;
};
Skips skips(const DsxTuning& t) {
#ifdef DSX_DIAG
  return {t.skip_hist, t.skip_row, t.skip_from};
#else
  (void)t;
  return {0, 0, 1000};
#endif
}

// The IN_KIND instantiation of a level kernel: 0 / 1 = the level reads (or finishes) uint16 / float32 pixels, 2 = it
// reads and writes the workspace only.  (The instantiations are named in the order 2, 0, 1 at every call: the order the
// compiler emits them in, which the device-code comparison of profiles/chain_stages_device_code.txt holds still.)
template <typename K>
K pixel_kernel(int in_dtype, K k_u16, K k_f32) {
  return in_dtype == DSX_U16 ? k_u16 : k_f32;
}
template <typename K>
K level_kernel(bool pixels, int in_dtype, K k_ws, K k_u16, K k_f32) {
  return pixels ? pixel_kernel(in_dtype, k_u16, k_f32) : k_ws;
}

// ---- stage 0: zero the control block --------------------------------------------------------------------------------
int stage_zero(const Chain& c) {
  dsx_ctx* ctx = c.ctx;
  const CohortView& v = c.v;
  const int nb = c.nb, Lc = std::max(1, ctx->plan.L);
  static_assert(sizeof(dsx::PlaneStats) == dsx::kPlaneStatsBytes, "dsx_chain.h counts the control block in these");
  const dsx::ZeroLaunch z = dsx::zero_launch(nb, Lc, (size_t)(uintptr_t)v.minmax);
  if (z.grid_x > 0) {
    hipLaunchKernelGGL(dsx::k_zero3, dim3(z.grid_x), dim3(256), 0, v.stream, (uint4*)v.stats, z.n0, (uint4*)v.minmax, z.n1,
                       (uint4*)v.hist, z.n2);
    DSX_HIP(hipGetLastError());
  } else {
    DSX_HIP(hipMemsetAsync(v.stats, 0, sizeof(dsx::PlaneStats) * nb, v.stream));
    DSX_HIP(hipMemsetAsync(v.minmax, 0, sizeof(unsigned) * 2 * Lc * (size_t)nb, v.stream));
    DSX_HIP(hipMemsetAsync(v.hist, 0, sizeof(unsigned) * 256 * Lc * nb, v.stream));
  }
  return DSX_OK;
}

// histograms of levels [l0, l1) in ONE launch (k_hist finds its level from the block index)
int hist_levels(const Chain& c, int l0, int l1, hipStream_t hs) {
  dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const Skips sk = skips(ctx->tune);
  if (!c.sh.thresholds) return DSX_OK;
  dsx::HistArgs a;
  memset(&a, 0, sizeof(a));
  a.ws = c.v.ws;
  a.ws_plane_stride = p.plane_floats;
  a.minmax = c.v.minmax;
  a.hist = c.v.hist;
  a.L = p.L;
  a.shared = ctx->stack_mode ? 1 : 0;
  int blocks = 0;
  for (int l = l0; l < l1 && l < sk.from; ++l) {
    if ((sk.hist >> l) & 1) continue;
    const dsx::LevelPlan& lp = p.lv[l];
    const int i = a.nlev++;
    a.lvl[i] = l;
    a.da_off[i] = lp.da_off;
    a.h[i] = lp.h; a.w[i] = lp.w; a.ld[i] = lp.ld;
    a.rows_per_block[i] = dsx::hist_rows_per_block(ctx->tune, lp.h, lp.w, c.nb);
    blocks += (lp.h + a.rows_per_block[i] - 1) / a.rows_per_block[i];
    a.blk_end[i] = blocks;
  }
  if (a.nlev == 0) return DSX_OK;
  LaunchScope ls(ctx, KC_HIST);
  hipLaunchKernelGGL(dsx::k_hist, dim3(blocks, c.nb), dim3(64 * dsx::kHistWaves), 0, hs, a);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

// the fields Fwd1Args and GenFwdArgs share: analysis level l (index) of the part
template <typename A>
void fill_fwd(A& a, const Chain& c, int l) {
  const dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const dsx::LevelPlan& lp = p.lv[l];
  memset(&a, 0, sizeof(a));
  a.in = c.d_in;
  a.in_plane_stride = (long long)p.H * p.W;
  a.ws = c.v.ws;
  a.ws_plane_stride = p.plane_floats;
  a.in_off = (l > 0) ? p.lv[l - 1].aa_off : 0;
  a.H = lp.hin; a.W = lp.win; a.ldin = lp.ldin;
  a.aa_off = lp.aa_off; a.da_off = lp.da_off;
  a.h = lp.h; a.w = lp.w; a.ld = lp.ld; a.lda = lp.lda;
  a.minmax = c.v.minmax;
  a.lvl = l; a.L = p.L;
  a.stats = c.v.stats;
  a.fg_cutoff = ctx->fg_cutoff;
  a.shared = ctx->stack_mode ? 1 : 0;
}

// ---- stage 1: forward transform --------------------------------------------------------------------------------------
// db3: k_fwd_march per level, levels 1 + 2 in ONE launch when the plane allows it (fuse12); any other wavelet: k_fwd_gen
// per level.  split: once levels 1 and 2 are complete their histograms start on the helper stream (ev[0] -> ev[1]).
int stage_forward(const Chain& c) {
  dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const CohortView& v = c.v;
  const dsx::ChainShape& sh = c.sh;
  hipStream_t s = v.stream;
  const int nb = c.nb;
  for (int l = 0; l < p.L; ++l) {
    if (sh.fuse12 && l == 1) continue;
    if (l >= skips(ctx->tune).from) continue;
    const dsx::LevelPlan& lp = p.lv[l];
    LaunchScope ls(ctx, l == 0 ? KC_FWD1 : KC_FWD);
    if (sh.generic) {
      dsx::GenFwdArgs g;
      fill_fwd(g, c, l);
      g.F = ctx->wl_len;
      memcpy(g.lo, ctx->wl[0], sizeof(float) * ctx->wl_len);
      memcpy(g.hi, ctx->wl[1], sizeof(float) * ctx->wl_len);
      const dim3 gg((lp.w + dsx::kGenTW - 1) / dsx::kGenTW, (lp.h + dsx::kGenTH - 1) / dsx::kGenTH, nb);
      auto kern = level_kernel(l == 0, c.in_dtype, dsx::k_fwd_gen<2>, dsx::k_fwd_gen<0>, dsx::k_fwd_gen<1>);
      hipLaunchKernelGGL(kern, gg, dim3(256), dsx::gen_fwd_lds_bytes(g.F), s, g);
      DSX_HIP(hipGetLastError());
      continue;
    }
    dsx::Fwd1Args f;
    fill_fwd(f, c, l);
    f.ablate = ctx->ablate;
    f.fg_cutoff_u16 = (unsigned)std::min(65536.0, std::max(0.0, ceil((double)ctx->fg_cutoff)));
    const bool fused = sh.fuse12 && l == 0;
    if (fused) {
      const dsx::LevelPlan& l2 = p.lv[1];
      f.aa2_off = l2.aa_off; f.da2_off = l2.da_off;
      f.h2 = l2.h; f.w2 = l2.w; f.ld2 = l2.ld; f.lda2 = l2.lda;
    }
    const dsx::MarchLaunch m = dsx::fwd_launch(p, sh, ctx->tune, ctx->cus, nb, v.alone, l);
    f.nstrips = m.nstrips; f.nseg = m.nseg; f.rows_per_seg = m.rows_per_seg;
    auto kern = (fused && m.wpb == 8) ? pixel_kernel(c.in_dtype, dsx::k_fwd_march<0, true, 8>, dsx::k_fwd_march<1, true, 8>)
                : fused ? pixel_kernel(c.in_dtype, dsx::k_fwd_march<0, true>, dsx::k_fwd_march<1, true>)
                : level_kernel(l == 0, c.in_dtype, dsx::k_fwd_march<2>, dsx::k_fwd_march<0>, dsx::k_fwd_march<1>);
    hipLaunchKernelGGL(kern, dim3(m.grid_x, nb), dim3(64 * m.wpb), 0, s, f);
    DSX_HIP(hipGetLastError());
    if (sh.split && l == 0) {  // levels 1 and 2 are complete: their histograms start now, on the helper stream
      DSX_HIP(hipEventRecord(v.ev[0], s));
      DSX_HIP(hipStreamWaitEvent(v.helper, v.ev[0], 0));
      if (int rc = hist_levels(c, 0, 2, v.helper)) return rc;
      DSX_HIP(hipEventRecord(v.ev[1], v.helper));
    }
  }
  return DSX_OK;
}

// ---- stage 2: thresholds ---------------------------------------------------------------------------------------------
// the histograms that did not go to the helper stream, k_otsu (config decision, threshold per level) and the cfg_used copy
int stage_thresholds(const Chain& c, int32_t* d_cfg_used) {
  dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const CohortView& v = c.v;
  hipStream_t s = v.stream;
  const int L = p.L;
  if (int rc = hist_levels(c, c.sh.split ? 2 : 0, L, s)) return rc;
  if (c.sh.split) DSX_HIP(hipStreamWaitEvent(s, v.ev[1], 0));  // histograms of levels 1, 2 (helper stream)
  if (L > 0 && c.sh.thresholds) {
    dsx::OtsuArgs a;
    a.stats = v.stats;
    a.npix = (double)p.H * (double)p.W;
    a.high_int = ctx->high_int;
    a.minmax = v.minmax;
    a.hist = v.hist;
    a.thr = v.thr;
    a.otsu = v.otsu;
    a.cfg = v.cfg;
    a.means = v.means;
    a.max_thr[0] = (float)ctx->cfg[0].max_threshold;
    a.max_thr[1] = (float)ctx->cfg[1].max_threshold;
    a.L = L;
    a.sticky = ctx->d_sticky;
    a.shared = ctx->stack_mode ? 1 : 0;
    LaunchScope ls(ctx, KC_OTSU);
    hipLaunchKernelGGL(dsx::k_otsu, dim3(L, c.nb), dim3(64), 0, s, a);
    DSX_HIP(hipGetLastError());
    if (d_cfg_used)
      DSX_HIP(hipMemcpyAsync(d_cfg_used, v.cfg, sizeof(int32_t) * c.nb, hipMemcpyDeviceToDevice, s));
  } else if (d_cfg_used) {
    DSX_HIP(hipMemsetAsync(d_cfg_used, 0, sizeof(int32_t) * c.nb, s));
  }
  return DSX_OK;
}

dsx::RowArgs row_args(const Chain& c, int l) {
  const dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const dsx::LevelPlan& lp = p.lv[l];
  dsx::RowArgs a;
  memset(&a, 0, sizeof(a));
  a.ws = c.v.ws;
  a.ws_plane_stride = p.plane_floats;
  a.da_off = lp.da_off;
  a.h = lp.h; a.w = lp.w; a.ld = lp.ld;
  a.thr = c.v.thr;
  a.cfg = c.v.cfg;
  a.lvl = l; a.L = p.L;
  a.lvl_active[0] = p.cfg_levels[0];
  a.lvl_active[1] = p.cfg_levels[1];
  a.M = lp.M; a.K = lp.K;
  a.npass = lp.npass;
  for (int i = 0; i < lp.npass; ++i) a.radix[i] = lp.radix[i];
  a.tw = (const float2*)(ctx->d_consts + lp.tw_off);
  a.g[0] = (const float2*)(ctx->d_consts + lp.g_off[0]);
  a.g[1] = (const float2*)(ctx->d_consts + lp.g_off[1]);
  a.kcut[0] = lp.kcut[0];
  a.kcut[1] = lp.kcut[1];
  a.inv_M = 1.0f / (float)lp.M;
  a.ablate = ctx->ablate;
  a.median_lockstep = ctx->tune.median_lockstep ? 1 : 0;
  return a;
}

// ---- stage 3: row filters --------------------------------------------------------------------------------------------
// split_inv: levels 1, 2 on the helper stream behind ev[2] ("thresholds are known"), ev[3] marks their end; the coarse
// levels on the part's own stream, in one merged launch where dsx::row_multi_takes says so.  With k_rowfinal level 1 is
// not launched here: *row1 carries its arguments to the final kernel.
int stage_rowfilters(const Chain& c, dsx::RowArgs* row1) {
  dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const CohortView& v = c.v;
  hipStream_t s = v.stream;
  const Skips sk = skips(ctx->tune);
  if (c.sh.split_inv) {
    DSX_HIP(hipEventRecord(v.ev[2], s));                  // thresholds are known
    DSX_HIP(hipStreamWaitEvent(v.helper, v.ev[2], 0));
  }
  memset(row1, 0, sizeof(*row1));
  dsx::RowMultiArgs multi;
  memset(&multi, 0, sizeof(multi));
  int multi_pairs[dsx::kRowMultiMax] = {};
  for (int l = 0; l < p.L && l < sk.from; ++l) {
    hipStream_t rs = (c.sh.split_inv && l < 2) ? v.helper : s;
    if ((sk.row >> l) & 1) continue;
    const dsx::RowArgs a = row_args(c, l);
    if (c.sh.rf_plan != 0 && l == 0) {
      *row1 = a;
      continue;
    }
    const int npairs = (a.h + 1) / 2;
    if (dsx::row_multi_takes(c.sh, rs == s, a.M, multi.nlev)) {
      multi_pairs[multi.nlev] = npairs;
      multi.lv[multi.nlev++] = a;
      continue;
    }
    LaunchScope ls(ctx, KC_ROW);
    DSX_HIP(dispatch_rowfilter(ctx->tune, a, npairs, c.nb, rs));
  }
  int multi_waves = 0;  // per plane, one row pair per wave
  for (int i = 0; i < multi.nlev; ++i) multi_waves += multi_pairs[i];
  if (multi.nlev == 1) {
    LaunchScope ls(ctx, KC_ROW);
    DSX_HIP(dispatch_rowfilter(ctx->tune, multi.lv[0], multi_pairs[0], c.nb, s));
  } else if (dsx::row_pack_runs(ctx->tune, multi.nlev, (long long)c.nb * multi_waves, ctx->cus)) {
    LaunchScope ls(ctx, KC_ROW);
    DSX_HIP(launch_rowfilter_pack(ctx->tune, multi, multi_pairs, c.nb, s));
    ++ctx->row_pack_launches;
  } else if (multi.nlev > 1) {
    LaunchScope ls(ctx, KC_ROW);
    DSX_HIP(launch_rowfilter_multi(multi, multi_pairs, c.nb, s));
  }
  if (c.sh.split_inv) DSX_HIP(hipEventRecord(v.ev[3], v.helper));
  return DSX_OK;
}

// the fields FinalArgs and GenInvArgs share: synthesis level l (index; -1: a plan without levels) of the part, the last
// one (l <= 0) writes the result
template <typename A>
void fill_inv(A& a, const Chain& c, int l) {
  const dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  memset(&a, 0, sizeof(a));
  a.ws = c.v.ws;
  a.ws_plane_stride = p.plane_floats;
  if (l >= 0) {
    const dsx::LevelPlan& lp = p.lv[l];
    a.c_off = lp.aa_off;
    a.d_off = lp.da_off;
    a.hc = lp.h; a.wc = lp.w; a.ldc = lp.lda; a.ldd = lp.ld;
    a.has_c = (l < p.L - 1) ? 1 : 0;
    a.has_pyr = 1;
  }
  if (l > 0) {
    const dsx::LevelPlan& lo = p.lv[l - 1];
    a.out_off = lo.aa_off;
    a.hout = lo.h; a.wout = lo.w; a.ldout = lo.lda;
  } else {
    a.img = c.d_in;
    a.img_plane_stride = (long long)p.H * p.W;
    a.H = p.H; a.W = p.W;
    a.out = c.d_out;
    a.out_plane_stride = (long long)p.Hout * p.Wout;
    a.hout = p.Hout; a.wout = p.Wout;
    a.out_dtype = (c.out_dtype == DSX_U16) ? 0 : 1;
    a.flat = ctx->d_flat;
    a.dark = ctx->d_dark;
    a.dark_ld = ctx->dark_w;
  }
}

// ---- stage 4: inverse transform of the Delta pyramid + finish ----------------------------------------------------------
// coarsest level first; level-2 synthesis inside the final kernel when the plane allows it (fuse21), the level-1 row filter
// too where k_rowfinal takes the shape (row1 from stage_rowfilters).  split_inv: the final kernel waits for ev[3].
int stage_inverse(const Chain& c, const dsx::RowArgs& row1) {
  dsx_ctx* ctx = c.ctx;
  const dsx::Plan& p = ctx->plan;
  const CohortView& v = c.v;
  const dsx::ChainShape& sh = c.sh;
  hipStream_t s = v.stream;
  const int L = p.L, nb = c.nb;
  for (int l = L - 1; l >= (L > 0 ? 0 : -1); --l) {
    if (sh.fuse21 && l == 1) continue;
    if (l >= skips(ctx->tune).from) continue;
    const bool last = (l <= 0);
    LaunchScope ls(ctx, last ? KC_FINAL : KC_INV);
    if (sh.generic) {
      dsx::GenInvArgs g;
      fill_inv(g, c, l);
      g.F = ctx->wl_len;
      memcpy(g.lo, ctx->wl[2], sizeof(float) * ctx->wl_len);
      memcpy(g.hi, ctx->wl[3], sizeof(float) * ctx->wl_len);
      const dim3 gg((g.wout + dsx::kGenOW - 1) / dsx::kGenOW, (g.hout + dsx::kGenOH - 1) / dsx::kGenOH, nb);
      auto kern = level_kernel(last, c.in_dtype, dsx::k_inv_gen<2>, dsx::k_inv_gen<0>, dsx::k_inv_gen<1>);
      hipLaunchKernelGGL(kern, gg, dim3(256), dsx::gen_inv_lds_bytes(g.F), s, g);
      DSX_HIP(hipGetLastError());
      continue;
    }
    dsx::FinalArgs f;
    fill_inv(f, c, l);
    if (!last) f.ws_out = v.ws;
    f.ablate = ctx->ablate;
    const dsx::MarchLaunch m = dsx::inv_launch(sh, ctx->tune, ctx->cus, nb, l, f.hout, f.wout);
    f.nstrips = m.nstrips; f.nseg = m.nseg; f.rows_per_seg = m.rows_per_seg;
    const bool fused = sh.fuse21 && last;
    if (last && sh.split_inv) DSX_HIP(hipStreamWaitEvent(s, v.ev[3], 0));  // Delta_1, Delta_2 (helper stream)
    if (fused) {
      const dsx::LevelPlan& l2 = p.lv[1];
      f.c2_off = l2.aa_off; f.d2_off = l2.da_off;
      f.hc2 = l2.h; f.wc2 = l2.w; f.ldc2 = l2.lda; f.ldd2 = l2.ld;
      f.has_c2 = (L > 2) ? 1 : 0;
      f.has_c = 1;
      f.pair_io = sh.pair_io ? 1 : 0;
    }
    if (fused && sh.rf_plan != 0) {
      dsx::RowFinalArgs rf;
      rf.r = row1;
      rf.f = f;
      DSX_HIP(launch_rowfinal(sh.rf_plan, rf, nb, s));
      continue;
    }
    auto kern = (fused && m.wpb == 8) ? pixel_kernel(c.in_dtype, dsx::k_inv_march<0, true, 8>, dsx::k_inv_march<1, true, 8>)
                : fused ? pixel_kernel(c.in_dtype, dsx::k_inv_march<0, true>, dsx::k_inv_march<1, true>)
                : level_kernel(last, c.in_dtype, dsx::k_inv_march<2>, dsx::k_inv_march<0>, dsx::k_inv_march<1>);
    hipLaunchKernelGGL(kern, dim3(m.grid_x, nb), dim3(64 * m.wpb), 0, s, f);
    DSX_HIP(hipGetLastError());
  }
  return DSX_OK;
}

// One cohort part of nb planes through the whole chain (asynchronous): the shape of the chain (dsx_chain.h: what is
// fused, what runs beside what), then its stages in launch order.  The helper-stream events of a split part: ev[0] /
// ev[1] around the wide levels' histograms (stage_forward -> stage_thresholds), ev[2] / ev[3] around their row filters
// (stage_rowfilters -> the final kernel of stage_inverse).
int run_cohort(dsx_ctx* ctx, const CohortView& v, const void* d_in, int in_dtype, int nb, void* d_out,
               int out_dtype, int32_t* d_cfg_used) {
  dsx::ChainCall call;
  call.in_u16 = in_dtype == DSX_U16;
  call.out_u16 = out_dtype == DSX_U16;
  call.nb = nb;
  call.aligned16 = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;
  call.bank = ctx->wl_len > 0;
  call.stop_after = ctx->stop_after;
  call.st_march = ctx->st_march;
  call.has_helper = v.helper != nullptr;
  call.alone = v.alone;
  const Chain c = {ctx, v, dsx::chain_shape(ctx->plan, ctx->tune, call), d_in, in_dtype, nb, d_out, out_dtype};
  if (int rc = stage_zero(c)) return rc;
  if (int rc = stage_forward(c)) return rc;
  if (int rc = stage_thresholds(c, d_cfg_used)) return rc;
  if (ctx->stop_after == 1) return DSX_OK;
  dsx::RowArgs row1;  // level 1, for k_rowfinal
  if (int rc = stage_rowfilters(c, &row1)) return rc;
  if (ctx->stop_after == 2) return DSX_OK;
  return stage_inverse(c, row1);
}

size_t elem_size(int dtype) { return dtype == DSX_U16 ? 2 : 4; }

// pointer, count and element-type check of the run entry points
int check_run_args(dsx_ctx* ctx, const void* in, const void* out, int n, int in_dtype, int out_dtype) {
  if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, DSX_EINVAL, "bad plane pointers / count");
  if ((in_dtype != DSX_U16 && in_dtype != DSX_F32) || (out_dtype != DSX_U16 && out_dtype != DSX_F32))
    return fail(ctx, DSX_EINVAL, "unknown element type");
  return DSX_OK;
}

// a staging buffer of dsx_run_host: at least `need` bytes
int grow_stage(dsx_ctx* ctx, void** buf, size_t* have, size_t need) {
  if (*have >= need) return DSX_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr; *have = 0;
  DSX_HIP(hipMalloc(buf, need));
  *have = need;
  return DSX_OK;
}

// a work buffer of the codec entry points on the device: at least `need` bytes.  The stream may still use the buffer
// it replaces, so it is drained first.
template <class T>
int grow_device(dsx_ctx* ctx, hipStream_t s, T** buf, size_t* have, size_t need, const char* message) {
  if (need <= *have) return DSX_OK;
  DSX_HIP(hipStreamSynchronize(s));
  if (*buf) DSX_HIP(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  if (hipMalloc(buf, need) != hipSuccess) return fail(ctx, DSX_ENOMEM, message);
  *have = need;
  return DSX_OK;
}

// the pack stage of dsx_blosc_encode_device_ex for the container C: sizes -> offsets, slots (or the source) -> frames
template <class C>
void launch_pack(hipStream_t s, const dsx::zenc::PackArgs& pa) {
  hipLaunchKernelGGL(dsx::zenc::k_pack_scan<C>, dim3(1), dim3(256), 0, s, pa);
  if (pa.n_chunks > 0)
    hipLaunchKernelGGL(dsx::zenc::k_pack_copy<C>, dim3((unsigned)(pa.n_chunks * pa.nblocks)), dim3(256), 0, s, pa);
}

// alone: the cohort runs as this ONE part (which may then use its helper stream: dsx::part_uses_helper)
CohortView make_view(dsx_ctx* ctx, int po, hipStream_t stream, int part = 0, bool alone = false) {
  const int Lc = ctx->plan.L > 0 ? ctx->plan.L : 1;
  CohortView v;
  v.stream = stream;
  v.helper = dsx::part_uses_helper(ctx->tune, alone, ctx->profiling || ctx->stop_after != 0) ? ctx->helper[part] : nullptr;
  v.alone = alone;
  v.ev = ctx->ev_h[part];
  v.ws = ctx->d_ws + (size_t)po * ctx->plan.plane_floats;
  v.stats = ctx->d_stats + po;
  v.minmax = ctx->d_minmax + (size_t)po * Lc * 2;
  v.hist = ctx->d_hist + (size_t)po * Lc * 256;
  v.thr = ctx->d_thr + (size_t)po * Lc;
  v.otsu = ctx->d_otsu + (size_t)po * Lc;
  v.cfg = ctx->d_cfg + po;
  v.means = ctx->d_means + 2 * (size_t)po;
  return v;
}

// n planes [H, W] -> [W, H] on stream s (dsx_rot90.h); dir +1: np.rot90, -1: its inverse
void rot_planes(hipStream_t s, const void* src, void* dst, int dtype, int n, int H, int W, int dir) {
  if (n <= 0) return;
  if (dtype == DSX_U16) dsx::rot::rot90_launch<uint16_t>(s, src, dst, n, H, W, dir);
  else dsx::rot::rot90_launch<float>(s, src, dst, n, H, W, dir);
}

// The rotation buffers of a rotated plan, at least need_in / need_out bytes.  Streams of an earlier run may still use
// the buffers they replace, so the context is drained first (use_main joins the parts).
int grow_rot(dsx_ctx* ctx, size_t need_in, size_t need_out) {
  if (need_in <= ctx->rot_in_bytes && need_out <= ctx->rot_out_bytes) return DSX_OK;
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  void** buf[2] = {&ctx->rot_in, &ctx->rot_out};
  size_t* have[2] = {&ctx->rot_in_bytes, &ctx->rot_out_bytes};
  const size_t need[2] = {need_in, need_out};
  for (int k = 0; k < 2; ++k) {
    if (need[k] <= *have[k]) continue;
    if (*buf[k]) (void)hipFree(*buf[k]);
    *buf[k] = nullptr;
    ctx->workspace_bytes -= *have[k];
    *have[k] = 0;
    if (hipMalloc(buf[k], need[k]) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, DSX_ENOMEM, "hipMalloc (rotation buffers of a rotated plan)");
    }
    *have[k] = need[k];
    ctx->workspace_bytes += need[k];
  }
  return DSX_OK;
}

// One part of a cohort of the log-space chain: planes [po, po + n) of the cohort.  With a rotated plan the part turns
// its planes into its slice of rot_in ahead of its first kernel and its result out of rot_out behind its last one, both
// on its own stream, so the parts overlap as they do without the rotation.  (A streaks plan rotates around its whole
// cohort instead, streaks_run: the chain of its march route runs over virtual planes that are rotated already.)
int run_part(dsx_ctx* ctx, const CohortView& v, int po, const void* d_in, int in_dtype, int n, void* d_out,
             int out_dtype, int32_t* d_cfg_used, size_t in_plane, size_t out_plane) {
  if (!ctx->rot || ctx->streaks) return run_cohort(ctx, v, d_in, in_dtype, n, d_out, out_dtype, d_cfg_used);
  const dsx::Plan& p = ctx->plan;
  char* ri = (char*)ctx->rot_in + po * in_plane;
  char* ro = (char*)ctx->rot_out + po * out_plane;
  rot_planes(v.stream, d_in, ri, in_dtype, n, ctx->rot_H, ctx->rot_W, +1);
  DSX_HIP(hipGetLastError());
  if (int rc = run_cohort(ctx, v, ri, in_dtype, n, ro, out_dtype, d_cfg_used)) return rc;
  if (ctx->stop_after != 0) return DSX_OK;  // (no result is made)
  rot_planes(v.stream, ro, d_out, out_dtype, n, p.Hout, p.Wout, -1);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

// An unsplit cohort through the graph cache (DSX_GRAPH=1, see dsx_ctx::GraphEntry): replay of a call seen before (same
// buffers, count and types under the current plan); first sight eager, second sight capture; a runtime that cannot
// capture falls back to eager launches for good.
int run_cohort_graphed(dsx_ctx* ctx, const CohortView& view, hipStream_t main, const void* d_in, int in_dtype, int nb,
                       void* d_out, int out_dtype, int32_t* d_cfg_used) {
  dsx_ctx::GraphEntry* hit = nullptr;
  for (auto& g : ctx->graphs)
    if (g.in == d_in && g.out == d_out && g.cfg == (const void*)d_cfg_used && g.n == nb && g.in_dtype == in_dtype &&
        g.out_dtype == out_dtype) { hit = &g; break; }
  if (!hit) {
    if ((int)ctx->graphs.size() >= dsx_ctx::kGraphSlots) {  // evict the least recently used tuple
      size_t lru = 0;
      for (size_t i = 1; i < ctx->graphs.size(); ++i)
        if (ctx->graphs[i].last_use < ctx->graphs[lru].last_use) lru = i;
      if (ctx->graphs[lru].exec) (void)hipGraphExecDestroy(ctx->graphs[lru].exec);
      ctx->graphs.erase(ctx->graphs.begin() + (long)lru);
    }
    ctx->graphs.push_back({d_in, d_out, (const void*)d_cfg_used, nb, in_dtype, out_dtype, 0, nullptr, 0});
    hit = &ctx->graphs.back();
  }
  hit->last_use = ++ctx->graph_clock;
  if (hit->exec) {
    ++ctx->graph_launches;
    DSX_HIP(hipGraphLaunch(hit->exec, main));
    return DSX_OK;
  }
  if (hit->seen++ == 0)  // first sight: eager (one-off calls never pay for a capture; function attributes get set)
    return run_cohort(ctx, view, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used);
  // second sight: capture the chain (the helper stream joins the capture through its fork event and is joined
  // back before the final kernel), instantiate, launch
  if (hipStreamBeginCapture(main, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    ctx->graph_mode = 0;
    return run_cohort(ctx, view, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used);
  }
  const int rc = run_cohort(ctx, view, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used);
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(main, &graph);
  hipGraphExec_t exec = nullptr;
  if (rc == DSX_OK && ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
    (void)hipGraphDestroy(graph);
    hit->exec = exec;
    ++ctx->graph_captures;
    ++ctx->graph_launches;
    DSX_HIP(hipGraphLaunch(exec, main));
    return DSX_OK;
  }
  // capture is not usable here: nothing has run yet -- fall back to eager launches for good
  (void)hipGetLastError();
  if (graph) (void)hipGraphDestroy(graph);
  ctx->graph_mode = 0;
  if (rc != DSX_OK) return rc;
  return run_cohort(ctx, view, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used);
}

// One cohort (<= max_batch planes), split into parts on the context's streams.
//
// Part 0 runs on the context stream, parts 1.. on the auxiliary streams behind a fork event.  The context
// stream does NOT wait for the other parts here: use_main() does that when an entry point needs the stream
// next.  If the call that follows is another split cohort with the same planes pointer, result pointer,
// count and element types (and nothing has been put on the context stream in between), every part is
// simply queued behind the same part of this call -- it reads the input nobody writes and rewrites its
// own slice of the workspace, control block and result -- so consecutive batches overlap instead of
// draining the chip at every call boundary.  Anything else joins first, then forks again.
int run_cohort_split(dsx_ctx* ctx, const void* d_in, int in_dtype, int nb, void* d_out, int out_dtype,
                     int32_t* d_cfg_used, size_t in_plane, size_t out_plane) {
  const int parts = dsx::cohort_parts(ctx->n_streams, nb, ctx->profiling || ctx->stop_after != 0 || ctx->stack_mode);
  const bool rotated = ctx->rot && !ctx->streaks;
  if (rotated)
    if (int rc = grow_rot(ctx, in_plane * ctx->max_batch, out_plane * ctx->max_batch)) return rc;
  if (parts <= 1) {
    hipStream_t main = use_main(ctx);  // joins whatever split cohort is still running
    const CohortView view = make_view(ctx, 0, main, 0, true);
    if (ctx->graph_mode == 0 || ctx->profiling || ctx->stop_after != 0 || ctx->ablate != 0 || rotated)  // (rotated: eager)
      return run_part(ctx, view, 0, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used, in_plane, out_plane);
    return run_cohort_graphed(ctx, view, main, d_in, in_dtype, nb, d_out, out_dtype, d_cfg_used);
  }
  const bool no_pipe = ctx->tune.no_pipeline;
  auto& ls = ctx->last_split;
  const bool in_out_disjoint = (const char*)d_in + nb * in_plane <= (const char*)d_out ||
                               (const char*)d_out + nb * out_plane <= (const char*)d_in;
  const bool same_call = !no_pipe && ctx->joins_pending == parts && ls.in == d_in && ls.out == d_out && ls.n == nb &&
                         ls.in_dtype == in_dtype && ls.out_dtype == out_dtype && ls.parts == parts &&
                         ls.cfg == (const void*)d_cfg_used && ls.main_ops == ctx->main_ops && in_out_disjoint;
  if (!same_call) {
    hipStream_t main = use_main(ctx);
    DSX_HIP(hipEventRecord(ctx->ev_fork, main));
  }
  const int per = (nb + parts - 1) / parts;
  for (int i = 0; i < parts; ++i) {
    const int po = i * per, n = std::min(per, nb - po);
    if (n <= 0) break;
    hipStream_t st = (i == 0) ? ctx->stream_ : ctx->aux[i];
    if (i > 0 && !same_call) DSX_HIP(hipStreamWaitEvent(st, ctx->ev_fork, 0));
    const int rc = run_part(ctx, make_view(ctx, po, st, i), po, (const char*)d_in + po * in_plane, in_dtype, n,
                            (char*)d_out + po * out_plane, out_dtype, d_cfg_used ? d_cfg_used + po : nullptr, in_plane,
                            out_plane);
    if (rc != DSX_OK) return rc;
    if (i > 0) DSX_HIP(hipEventRecord(ctx->ev_join[i], st));
  }
  ctx->joins_pending = parts;
  ls.in = d_in; ls.out = d_out; ls.cfg = d_cfg_used;
  ls.n = nb; ls.in_dtype = in_dtype; ls.out_dtype = out_dtype; ls.parts = parts;
  ls.main_ops = ctx->main_ops;
  return DSX_OK;
}

// Value errors of planes that went through the asynchronous device-buffer path (see dsx_ctx::h_sticky): reported once,
// by the first synchronising entry point after the kernels that found them.
int check_sticky(dsx_ctx* ctx) {
  if (!ctx->h_sticky) return DSX_OK;
  // one atomic exchange: a kernel of another stream may be storing its 1 right now -- read-then-clear could lose it
  const unsigned f = __atomic_exchange_n(ctx->h_sticky, 0u, __ATOMIC_ACQ_REL);
  if (f == 0u) return DSX_OK;
  return fail(ctx, DSX_EVALUE, "a plane of an earlier dsx_run_device call: autodetected range of [nan, nan] is not finite "
                               "(a float32 pixel is NaN, infinite or <= -1); that plane's result is not valid");
}

// ---- dual-band filter (dsx_plan_streaks) ----------------------------------------------------------------------------
void free_streaks(dsx_ctx* c) {
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(c->st_ws); c->st_ws = nullptr;
  fr(c->st_mat); c->st_mat = nullptr;
  fr(c->st_mm); c->st_mm = nullptr;
  fr(c->st_hist); c->st_hist = nullptr;
  fr(c->st_t); c->st_t = nullptr;
  fr(c->st_info); c->st_info = nullptr;
  fr(c->st_vin); c->st_vin = nullptr;
  fr(c->st_vout); c->st_vout = nullptr;
  fr(c->st_flat); c->st_flat = nullptr;
  fr(c->st_dark); c->st_dark = nullptr;
  c->st_opts = false;
  c->st_mode = dsx::st::kStBoth;
  c->st_R = 0;
  c->st_march = false;
  c->streaks = false;
}

__global__ __launch_bounds__(256) void k_st_mminit(unsigned* mm, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { mm[2 * i] = 0xffffffffu; mm[2 * i + 1] = 0u; }
}

inline unsigned st_blocks(size_t total) { return (unsigned)((total + 255) / 256); }

template <typename TI, typename TO>
void st_final(hipStream_t s, const dsx::st::StreaksPlan& p, const void* in, const float* r, int nb, const float* t,
              void* out) {
  const size_t total = (size_t)p.H * p.W * nb;
  dsx::st::k_st_final<TI, TO><<<st_blocks(total), 256, 0, s>>>((const TI*)in, r, nb, nb, p.H, p.W, p.Hp, p.Wp,
                                                               p.bands, t, 1.0f / p.crossover, (TO*)out);
}

// Threshold per plane of a cohort into ctx->st_t (both routes)
int streaks_threshold(dsx_ctx* ctx, hipStream_t s, const void* d_in, bool u16, int nb) {
  using namespace dsx::st;
  const StreaksPlan& p = ctx->sp;
  const size_t px = (size_t)p.H * p.W;
  if (p.otsu) {
    k_st_mminit<<<st_blocks(nb), 256, 0, s>>>(ctx->st_mm, nb);
    DSX_HIP(hipMemsetAsync(ctx->st_hist, 0, sizeof(unsigned) * kStBins * nb, s));
    const unsigned bx = (unsigned)std::max<size_t>(1, std::min<size_t>(128, px / (256 * 32)));
    const dim3 g(bx, nb);
    if (u16) {
      k_st_minmax<uint16_t><<<g, 256, 0, s>>>((const uint16_t*)d_in, px, ctx->st_mm);
      k_st_hist<uint16_t><<<g, 256, 0, s>>>((const uint16_t*)d_in, px, ctx->st_mm, ctx->st_hist);
      k_st_otsu<true><<<nb, kOtsuThreads, 0, s>>>(ctx->st_mm, ctx->st_hist, ctx->st_t, ctx->st_info);
    } else {
      k_st_minmax<float><<<g, 256, 0, s>>>((const float*)d_in, px, ctx->st_mm);
      k_st_hist<float><<<g, 256, 0, s>>>((const float*)d_in, px, ctx->st_mm, ctx->st_hist);
      k_st_otsu<false><<<nb, kOtsuThreads, 0, s>>>(ctx->st_mm, ctx->st_hist, ctx->st_t, ctx->st_info);
    }
  } else {
    k_st_fill<<<st_blocks(nb), 256, 0, s>>>(ctx->st_t, nb, p.threshold);
  }
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

template <typename TI, typename TV>
void st_bands(hipStream_t s, dim3 g, bool vec, const void* in, size_t px, int bands, int clip, const float* t, void* v,
              unsigned* sticky) {
  using namespace dsx::st;
  if (vec) k_st_bands<TI, TV, 4><<<g, 256, 0, s>>>((const TI*)in, px, bands, clip, t, (TV*)v, sticky);
  else k_st_bands<TI, TV, 1><<<g, 256, 0, s>>>((const TI*)in, px, bands, clip, t, (TV*)v, sticky);
}

// The blend of a plan with options (dsx_plan_streaks_opts) for one cohort, on either route: ld says where the bands
// are, band_pitch is their row pitch
template <typename L>
void st_blendx(dsx_ctx* ctx, hipStream_t s, const L& ld, int band_pitch, const void* d_in, int in_dtype, const float* r,
               int nb, void* d_out, int out_dtype) {
  using namespace dsx::st;
  const StreaksPlan& p = ctx->sp;
  BlendArgs a;
  a.in = d_in; a.r = r; a.out = d_out; a.t = ctx->st_t;
  a.flat = ctx->st_flat; a.dark = ctx->st_dark; a.dark_w = ctx->st_dark_w;
  a.H = p.H; a.W = p.W; a.mode = ctx->st_mode;
  a.R = ctx->st_mode == kStSingle ? 0 : ctx->st_R;
  a.inv_crossover = 1.0f / p.crossover;
  memcpy(a.taps, ctx->st_taps, sizeof(a.taps));
  auto aligned = [](const void* q, size_t n) { return ((uintptr_t)q % n) == 0; };
  a.vec = (p.W % 4) == 0 && (band_pitch % 4) == 0 && aligned(d_in, 4 * elem_size(in_dtype)) &&
          aligned(d_out, 4 * elem_size(out_dtype)) && aligned(r, 16) &&
          (a.flat == nullptr || ((a.dark_w % 4) == 0 && aligned(a.flat, 16) && aligned(a.dark, 16)));
  const dim3 g((unsigned)((p.W + kBtW - 1) / kBtW), (unsigned)((p.H + kBtH - 1) / kBtH), (unsigned)nb);
  const bool smooth = a.R > 0, u16 = in_dtype == DSX_U16;
#define DSX_ST_BX(TI, TO)                                                     \
  do {                                                                        \
    if (smooth) k_st_blendx<L, TI, TO, true><<<g, 256, 0, s>>>(a, ld);        \
    else k_st_blendx<L, TI, TO, false><<<g, 256, 0, s>>>(a, ld);              \
  } while (0)
  if (u16 && out_dtype == DSX_U16) DSX_ST_BX(uint16_t, uint16_t);
  else if (u16) DSX_ST_BX(uint16_t, float);
  else if (out_dtype == DSX_U16) DSX_ST_BX(float, uint16_t);
  else DSX_ST_BX(float, float);
#undef DSX_ST_BX
}
template <typename TI, typename TO>
void st_blend(hipStream_t s, dim3 g, bool vec, const void* in, const float* r, size_t px, int bands, const float* t,
              float inv_crossover, void* out) {
  using namespace dsx::st;
  if (vec) k_st_blend<TI, TO, 4><<<g, 256, 0, s>>>((const TI*)in, r, px, bands, t, inv_crossover, (TO*)out);
  else k_st_blend<TI, TO, 1><<<g, 256, 0, s>>>((const TI*)in, r, px, bands, t, inv_crossover, (TO*)out);
}

// One cohort of the march route: threshold, band planes and the row filters' thr / cfg on the context stream, the
// log-space chain over the virtual planes on the sub-cohort streams (run_cohort_split forks them behind an event of
// the context stream), the blend on the context stream again, behind the join events (use_main).
int streaks_cohort_march(dsx_ctx* ctx, const void* d_in, int in_dtype, int nb, void* d_out, int out_dtype) {
  using namespace dsx::st;
  const StreaksPlan& p = ctx->sp;
  const bool u16 = in_dtype == DSX_U16;
  const size_t px = (size_t)p.H * p.W;
  const int P = p.bands * nb, Lc = std::max(1, ctx->plan.L);
  const int vdtype = u16 ? ctx->st_vdtype : DSX_F32;
  // use_main joins the parts of the cohort before (they read the buffers written below) and counts as an operation on
  // the context stream, so run_cohort_split forks anew instead of queueing its parts behind their predecessors
  hipStream_t s = use_main(ctx);
  if (int rc = streaks_threshold(ctx, s, d_in, u16, nb)) return rc;
  k_st_chainfill<<<st_blocks((size_t)std::max(P * Lc, P)), 256, 0, s>>>(ctx->d_thr, P * Lc, ctx->d_cfg, P, p.bands,
                                                                        p.clip == kStBg ? 1 : 0);
  const dim3 g((unsigned)std::max<size_t>(1, std::min<size_t>(1024, px / (256 * 4 * 4))), nb);
  const size_t esz = elem_size(in_dtype);
  const bool vec_in = ((uintptr_t)d_in % (4 * esz)) == 0;
  if (!u16) st_bands<float, float>(s, g, vec_in, d_in, px, p.bands, p.clip, ctx->st_t, ctx->st_vin, ctx->d_sticky);
  else if (vdtype == DSX_U16) st_bands<uint16_t, uint16_t>(s, g, vec_in, d_in, px, p.bands, p.clip, ctx->st_t, ctx->st_vin, nullptr);
  else st_bands<uint16_t, float>(s, g, vec_in, d_in, px, p.bands, p.clip, ctx->st_t, ctx->st_vin, nullptr);
  DSX_HIP(hipGetLastError());
  if (int rc = run_cohort_split(ctx, ctx->st_vin, vdtype, P, ctx->st_vout, DSX_F32, nullptr, px * elem_size(vdtype),
                                px * sizeof(float)))
    return rc;
  s = use_main(ctx);
  const bool vec = vec_in && ((uintptr_t)d_out % (4 * elem_size(out_dtype))) == 0;
  const float ic = 1.0f / p.crossover;
  if (ctx->st_opts) st_blendx(ctx, s, StMarchBands{p.bands, p.W, px}, p.W, d_in, in_dtype, ctx->st_vout, nb, d_out, out_dtype);
  else if (u16 && out_dtype == DSX_U16) st_blend<uint16_t, uint16_t>(s, g, vec, d_in, ctx->st_vout, px, p.bands, ctx->st_t, ic, d_out);
  else if (u16) st_blend<uint16_t, float>(s, g, vec, d_in, ctx->st_vout, px, p.bands, ctx->st_t, ic, d_out);
  else if (out_dtype == DSX_U16) st_blend<float, uint16_t>(s, g, vec, d_in, ctx->st_vout, px, p.bands, ctx->st_t, ic, d_out);
  else st_blend<float, float>(s, g, vec, d_in, ctx->st_vout, px, p.bands, ctx->st_t, ic, d_out);
  DSX_HIP(hipGetLastError());
  ctx->last_n = nb;
  return DSX_OK;
}

// One cohort (nb <= max_batch planes) of the dual-band filter on stream s.
int streaks_cohort(dsx_ctx* ctx, const void* d_in, int in_dtype, int nb, void* d_out, int out_dtype) {
  using namespace dsx::st;
  if (ctx->st_march) return streaks_cohort_march(ctx, d_in, in_dtype, nb, d_out, out_dtype);
  const StreaksPlan& p = ctx->sp;
  hipStream_t s = use_main(ctx);
  const size_t px = (size_t)p.H * p.W;
  const bool u16 = in_dtype == DSX_U16;
  // 1. threshold per plane
  if (int rc = streaks_threshold(ctx, s, d_in, u16, nb)) return rc;
  // 2. log(1 + band) of the padded plane
  float* ws = ctx->st_ws;
  const int P = p.bands * nb;  // workspace planes of this cohort, band-major (v = band * nb + plane)
  {
    const size_t total = (size_t)p.Hp * p.Wp * nb * p.bands;
    if (u16)
      k_st_prep<uint16_t><<<st_blocks(total), 256, 0, s>>>((const uint16_t*)d_in, nb, nb, p.H, p.W, p.Hp, p.Wp,
                                                           p.bands, p.clip, ctx->st_t, ws + p.y, ctx->d_sticky);
    else
      k_st_prep<float><<<st_blocks(total), 256, 0, s>>>((const float*)d_in, nb, nb, p.H, p.W, p.Hp, p.Wp, p.bands,
                                                        p.clip, ctx->st_t, ws + p.y, ctx->d_sticky);
  }
  // 3. analysis: axis 0 into the temporaries, axis 1 into approx / cV (from lo) and cH / cD (from hi)
  int h = p.Hp, w = p.Wp;
  size_t src = p.y;
  for (int l = 0; l < p.L; ++l) {
    const StLevel& v = p.lv[l];
    // every kernel writes its outputs dense: [P][rows][columns]
    const size_t ps_in = (size_t)h * w;
    k_st_dwt<0><<<st_blocks((size_t)v.h * w * P), 256, 0, s>>>(ws + src, P, h, w, w, ps_in, ws + p.t0, ws + p.t1, p.F,
                                                               p.dec);
    const size_t ps_t = (size_t)v.h * w;
    k_st_dwt<1><<<st_blocks((size_t)v.h * v.w * P), 256, 0, s>>>(ws + p.t0, P, v.h, w, w, ps_t, ws + v.a, ws + v.cv,
                                                                 p.F, p.dec);
    k_st_dwt<1><<<st_blocks((size_t)v.h * v.w * P), 256, 0, s>>>(ws + p.t1, P, v.h, w, w, ps_t, ws + v.ch, ws + v.cd,
                                                                 p.F, p.dec);
    src = v.a;
    h = v.h;
    w = v.w;
  }
  // 4. row filter of every cH: per level and band over the nb planes of that band, Z = cH U into the first temporary
  //    (free between analysis and synthesis), then cH' = cH + Z V
  for (int l = 0; l < p.L; ++l) {
    const StLevel& v = p.lv[l];
    const size_t pl = (size_t)v.h * v.w;
    const int R = nb * v.h;
    for (int b = 0; b < p.bands; ++b) {
      const int K = v.rank[b];
      const float* U = ctx->st_mat + v.mat[b];
      const float* V = U + (size_t)v.w * K;
      const float* X = ws + v.ch + (size_t)b * nb * pl;
      k_st_rowmat<<<dim3((K + kMmT - 1) / kMmT, (R + kMmT - 1) / kMmT), 256, 0, s>>>(X, U, nullptr, ws + p.t0, R, v.w, K);
      k_st_rowmat<<<dim3((v.w + kMmT - 1) / kMmT, (R + kMmT - 1) / kMmT), 256, 0, s>>>(
          ws + p.t0, V, X, ws + v.cf + (size_t)b * nb * pl, R, K, v.w);
    }
  }
  // 5. synthesis, coarsest level first: axis 1 (approx + cV, filtered cH + cD), then axis 0
  for (int l = p.L - 1; l >= 0; --l) {
    const StLevel& v = p.lv[l];
    const size_t pl = (size_t)v.h * v.w;
    const size_t pa = (size_t)v.rh * v.rw;  // approx: forward output (top level) or the rebuild of level l + 1
    const int wo = 2 * v.w - p.F + 2, ho = 2 * v.h - p.F + 2;
    k_st_idwt<1><<<st_blocks((size_t)v.h * wo * P), 256, 0, s>>>(ws + v.a, v.rw, pa, ws + v.cv, v.w, pl, P, v.h, v.w,
                                                                 ws + p.t0, p.F, p.rec);
    k_st_idwt<1><<<st_blocks((size_t)v.h * wo * P), 256, 0, s>>>(ws + v.cf, v.w, pl, ws + v.cd, v.w, pl, P, v.h, v.w,
                                                                 ws + p.t1, p.F, p.rec);
    const size_t pt = (size_t)v.h * wo;
    float* dst = l == 0 ? ws + p.y : ws + p.lv[l - 1].a;
    k_st_idwt<0><<<st_blocks((size_t)ho * wo * P), 256, 0, s>>>(ws + p.t0, wo, pt, ws + p.t1, wo, pt, P, v.h, wo, dst,
                                                                p.F, p.rec);
  }
  // 6. exp(r) - 1, blend, crop, store
  if (ctx->st_opts) st_blendx(ctx, s, StGenericBands{nb, p.Hp, p.Wp}, p.Wp, d_in, in_dtype, ws + p.y, nb, d_out, out_dtype);
  else if (u16 && out_dtype == DSX_U16) st_final<uint16_t, uint16_t>(s, p, d_in, ws + p.y, nb, ctx->st_t, d_out);
  else if (u16) st_final<uint16_t, float>(s, p, d_in, ws + p.y, nb, ctx->st_t, d_out);
  else if (out_dtype == DSX_U16) st_final<float, uint16_t>(s, p, d_in, ws + p.y, nb, ctx->st_t, d_out);
  else st_final<float, float>(s, p, d_in, ws + p.y, nb, ctx->st_t, d_out);
  DSX_HIP(hipGetLastError());
  ctx->last_n = nb;
  return DSX_OK;
}

// ---- light-sheet background mode (dsx_plan_lightsheet) ---------------------------------------------------------------
void free_lightsheet(dsx_ctx* c) {
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(c->ls_edges); c->ls_edges = nullptr;
  fr(c->ls_back); c->ls_back = nullptr;
  fr(c->ls_q); c->ls_q = nullptr;
  fr(c->ls_ls); c->ls_ls = nullptr;
  fr(c->ls_bg); c->ls_bg = nullptr;
  c->lightsheet = false;
}

// One cohort of a light-sheet plan on the context stream: quantise, the 1 x A filter, the B x B filter with step 3
int lightsheet_cohort(dsx_ctx* ctx, const void* d_in, int in_dtype, int nb, void* d_out, int out_dtype) {
  using namespace dsx::ls;
  if (in_dtype != DSX_U16) return fail(ctx, DSX_EINVAL, "the light-sheet plan takes uint16 planes only");
  hipStream_t s = use_main(ctx);
  const int H = ctx->ls_H, W = ctx->ls_W, A = ctx->ls_A, B = ctx->ls_B;
  const size_t rows = (size_t)nb * H, total = rows * W;
  const uint16_t* x = (const uint16_t*)d_in;
  k_ls_quant<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(x, total, ctx->ls_edges, ctx->ls_q);
  const size_t runs = rows * ((W + kLsRun - 1) / kLsRun);
  if (A <= 255)
    k_ls_row<uint8_t, 128><<<(unsigned)((runs + 127) / 128), 128, 0, s>>>(ctx->ls_q, ctx->ls_ls, rows, W, A, ctx->ls_p);
  else
    k_ls_row<uint16_t, 64><<<(unsigned)((runs + 63) / 64), 64, 0, s>>>(ctx->ls_q, ctx->ls_ls, rows, W, A, ctx->ls_p);
  const int S = bg_strip(B);
  const dim3 grid((unsigned)((W + S - 1) / S), (unsigned)((H + kLsRows - 1) / kLsRows), (unsigned)nb);
  const size_t lds = bg_lds_bytes(W, B);
  if (out_dtype == DSX_U16) {
    DSX_HIP(raise_lds_limit<k_ls_bg<uint16_t>>());
    k_ls_bg<uint16_t><<<grid, kLsBgThreads, lds, s>>>(x, ctx->ls_q, ctx->ls_ls, ctx->ls_bg, (uint16_t*)d_out, ctx->ls_back,
                                                      H, W, B, S, ctx->ls_p, ctx->ls_lambda);
  } else {
    DSX_HIP(raise_lds_limit<k_ls_bg<float>>());
    k_ls_bg<float><<<grid, kLsBgThreads, lds, s>>>(x, ctx->ls_q, ctx->ls_ls, ctx->ls_bg, (float*)d_out, ctx->ls_back, H, W,
                                                   B, S, ctx->ls_p, ctx->ls_lambda);
  }
  DSX_HIP(hipGetLastError());
  ctx->last_n = nb;
  return DSX_OK;
}

// dsx_run_host (host = true: staged through the context's device buffers) / dsx_run_device of a streaks plan or a
// light-sheet plan: planes of H x W (the plan's own, rotated, geometry), cohorts of B planes through `run_one`
typedef int (*cohort_fn)(dsx_ctx*, const void*, int, int, void*, int);
int cohort_run(dsx_ctx* ctx, int H, int W, int B, cohort_fn run_one, const void* in, int in_dtype, int n, void* out,
               int out_dtype, bool host) {
  if (int rc = check_run_args(ctx, in, out, n, in_dtype, out_dtype)) return rc;
  DSX_HIP(hipSetDevice(ctx->device));
  const size_t in_plane = (size_t)H * W * elem_size(in_dtype);
  const size_t out_plane = (size_t)H * W * elem_size(out_dtype);
  if (host) {
    if (int rc = grow_stage(ctx, &ctx->d_stage_in, &ctx->stage_in_bytes, in_plane * B)) return rc;
    if (int rc = grow_stage(ctx, &ctx->d_stage_out, &ctx->stage_out_bytes, out_plane * B)) return rc;
  }
  if (ctx->rot)
    if (int rc = grow_rot(ctx, in_plane * B, out_plane * B)) return rc;
  // A rotated plan (H x W is the rotated geometry, H == rot_W): the cohort is turned into rot_in on the context stream,
  // filtered there into rot_out and turned back into the caller's buffer.
  auto cohort = [&](const void* d_src, int nb, void* d_dst) -> int {
    if (!ctx->rot) return run_one(ctx, d_src, in_dtype, nb, d_dst, out_dtype);
    rot_planes(use_main(ctx), d_src, ctx->rot_in, in_dtype, nb, ctx->rot_H, ctx->rot_W, +1);
    if (int rc = run_one(ctx, ctx->rot_in, in_dtype, nb, ctx->rot_out, out_dtype)) return rc;
    rot_planes(use_main(ctx), ctx->rot_out, d_dst, out_dtype, nb, H, W, -1);
    DSX_HIP(hipGetLastError());
    return DSX_OK;
  };
  if (host) {  // a value error of an earlier asynchronous call is reported now, not wiped by this call's check
    DSX_HIP(hipStreamSynchronize(use_main(ctx)));
    if (int rc = check_sticky(ctx)) return rc;
  }
  for (int start = 0; start < n; start += B) {
    const int nb = std::min(B, n - start);
    const char* src = (const char*)in + start * in_plane;
    char* dst = (char*)out + start * out_plane;
    if (host) {
      DSX_HIP(hipMemcpyAsync(ctx->d_stage_in, src, in_plane * nb, hipMemcpyHostToDevice, use_main(ctx)));
      if (int rc = cohort(ctx->d_stage_in, nb, ctx->d_stage_out)) return rc;
      DSX_HIP(hipMemcpyAsync(dst, ctx->d_stage_out, out_plane * nb, hipMemcpyDeviceToHost, use_main(ctx)));
      DSX_HIP(hipStreamSynchronize(use_main(ctx)));
      if (ctx->h_sticky && __atomic_exchange_n(ctx->h_sticky, 0u, __ATOMIC_ACQ_REL) != 0u)
        return fail(ctx, DSX_EVALUE, "a plane of " + std::to_string(start) + " .. " + std::to_string(start + nb - 1) +
                                         ": autodetected range of [nan, nan] is not finite (a pixel is NaN, infinite "
                                         "or <= -1)");
    } else if (int rc = cohort(src, nb, dst)) {
      return rc;
    }
  }
  return DSX_OK;
}

int streaks_run(dsx_ctx* ctx, const void* in, int in_dtype, int n, void* out, int out_dtype, bool host) {
  return cohort_run(ctx, ctx->sp.H, ctx->sp.W, ctx->sp.B, streaks_cohort, in, in_dtype, n, out, out_dtype, host);
}

int lightsheet_run(dsx_ctx* ctx, const void* in, int in_dtype, int n, void* out, int out_dtype, bool host) {
  if (in_dtype != DSX_U16) return fail(ctx, DSX_EINVAL, "the light-sheet plan takes uint16 planes only");
  return cohort_run(ctx, ctx->ls_H, ctx->ls_W, ctx->max_batch, lightsheet_cohort, in, in_dtype, n, out, out_dtype, host);
}

}  // namespace

extern "C" {

int dsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* dsx_last_error(const dsx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int dsx_init(int device, dsx_ctx** out_ctx) {
  if (!out_ctx) { g_init_error = "out_ctx is NULL"; return DSX_EINVAL; }
  *out_ctx = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_init_error = std::string("no HIP device available: ") + hipGetErrorString(e);
    return DSX_EHIP;
  }
  if (device < 0 || device >= n) { g_init_error = "device index out of range"; return DSX_EINVAL; }
  e = hipSetDevice(device);
  if (e != hipSuccess) { g_init_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return DSX_EHIP; }
  dsx_ctx* c = new dsx_ctx();
  c->device = device;
  dsx::read_tuning(c->tune);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = cus;
#ifdef DSX_DIAG
  if (const char* ab = getenv("DSX_ABLATE")) c->ablate = atoi(ab);
#endif
  if (const char* gm = getenv("DSX_GRAPH")) c->graph_mode = atoi(gm) != 0 ? 1 : 0;
  if (const char* ns = getenv("DSX_STREAMS")) c->n_streams = std::max(1, std::min(atoi(ns), (int)dsx_ctx::kMaxStreams));
  // DSX_PRIO=p0,p1,...: stream priority per sub-cohort stream (experiment hook; default: all equal)
  int prio[dsx_ctx::kMaxStreams] = {};
  if (const char* pr = getenv("DSX_PRIO")) {
    int i = 0;
    for (const char* q = pr; *q && i < dsx_ctx::kMaxStreams; ++i) {
      prio[i] = atoi(q);
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
  }
  e = hipStreamCreateWithPriority(&c->stream_, hipStreamNonBlocking, prio[0]);
  for (int i = 1; i < dsx_ctx::kMaxStreams && e == hipSuccess; ++i) {
    e = hipStreamCreateWithPriority(&c->aux[i], hipStreamNonBlocking, prio[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&c->copy_stream[i], hipStreamNonBlocking);
  for (int i = 0; i < dsx_ctx::kMaxStreams && e == hipSuccess; ++i) {
    e = hipStreamCreateWithFlags(&c->helper[i], hipStreamNonBlocking);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&c->ev_h[i][k], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_xs, hipEventDisableTiming);
  for (int i = 0; i < dsx_ctx::kEventSlots && e == hipSuccess; ++i)
    e = hipEventCreateWithFlags(&c->ev_slot[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_sticky, 64, hipHostMallocMapped);
  if (e == hipSuccess) {
    *c->h_sticky = 0u;
    e = hipHostGetDevicePointer((void**)&c->d_sticky, c->h_sticky, 0);
  }
  if (e == hipSuccess) e = hipEventCreate(&c->t0);
  if (e == hipSuccess) e = hipEventCreate(&c->t1);
  if (e != hipSuccess) {
    g_init_error = std::string("stream/event creation: ") + hipGetErrorString(e);
    delete c;
    return DSX_EHIP;
  }
  *out_ctx = c;
  return DSX_OK;
}

void dsx_destroy(dsx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(use_main(ctx));
  (void)dsx_comm_destroy(ctx);
  for (auto& r : ctx->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  free_plan_buffers(ctx);
  free_streaks(ctx);
  free_lightsheet(ctx);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  for (int i = 1; i < dsx_ctx::kMaxStreams; ++i) {
    if (ctx->aux[i]) { (void)hipStreamSynchronize(ctx->aux[i]); (void)hipStreamDestroy(ctx->aux[i]); }
    if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  for (int i = 0; i < dsx_ctx::kMaxStreams; ++i) {
    if (ctx->helper[i]) { (void)hipStreamSynchronize(ctx->helper[i]); (void)hipStreamDestroy(ctx->helper[i]); }
    for (int k = 0; k < 4; ++k) if (ctx->ev_h[i][k]) (void)hipEventDestroy(ctx->ev_h[i][k]);
  }
  for (int i = 0; i < 2; ++i)
    if (ctx->copy_stream[i]) { (void)hipStreamSynchronize(ctx->copy_stream[i]); (void)hipStreamDestroy(ctx->copy_stream[i]); }
  if (ctx->h_sticky) (void)hipHostFree(ctx->h_sticky);
  if (ctx->zenc_slots) (void)hipFree(ctx->zenc_slots);
  if (ctx->zenc_sizes) (void)hipFree(ctx->zenc_sizes);
  if (ctx->zenc_lits) (void)hipFree(ctx->zenc_lits);
  if (ctx->zdec_scratch) (void)hipFree(ctx->zdec_scratch);
  if (ctx->volhist) (void)hipFree(ctx->volhist);
  if (ctx->ev_xs) (void)hipEventDestroy(ctx->ev_xs);
  for (int i = 0; i < dsx_ctx::kEventSlots; ++i)
    if (ctx->ev_slot[i]) (void)hipEventDestroy(ctx->ev_slot[i]);
  if (ctx->stream_) (void)hipStreamDestroy(ctx->stream_);
  delete ctx;
}

namespace {
// The log-space chain of ctx->cfg[0 / 1] for planes of height x width, max_batch planes per cohort: plan, workspace,
// control block, constants and shading.  dsx_plan, and the march route of dsx_plan_streaks_ex (whose planes are the
// virtual band planes).  The context's earlier plan has been freed.
int plan_chain(dsx_ctx* ctx, int height, int width, int max_batch, bool bank, double microscope_high_int,
               const float* flat, const float* dark, int dark_h, int dark_w);
int rotated_shading_host(dsx_ctx* ctx, const float* flat, const float* dark, int dark_h, int dark_w);
}  // namespace

int dsx_plan(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_cfg* cells_config,
             const dsx_cfg* no_cells_config, double microscope_high_int, const float* flat,
             const float* dark, int dark_h, int dark_w) {
  if (!ctx) return DSX_EINVAL;
  if (!cells_config || !no_cells_config) return fail(ctx, DSX_EINVAL, "config is NULL");
  if (max_batch < 1) return fail(ctx, DSX_EINVAL, "max_batch must be >= 1");
  if ((flat == nullptr) != (dark == nullptr))
    return fail(ctx, DSX_EINVAL, "flatfield and darkfield must be given together");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  free_plan_buffers(ctx);
  free_streaks(ctx);
  free_lightsheet(ctx);

  const dsx_cfg* src[2] = {no_cells_config, cells_config};  // index 1 == cells_config
  for (int c = 0; c < 2; ++c) {
    // both configs run through ONE decomposition (the config is only decided once the level-1 statistic is known)
    if (src[c]->wavelet != DSX_WAVELET_DB3 && src[c]->wavelet != DSX_WAVELET_BANK)
      return fail(ctx, DSX_EINVAL, "unknown wavelet id");
    if (src[c]->wavelet != src[0]->wavelet)
      return fail(ctx, DSX_EINVAL, "cells_config and no_cells_config must name the same wavelet");
    ctx->cfg[c].level = src[c]->level;
    ctx->cfg[c].sigma = src[c]->sigma;
    ctx->cfg[c].max_threshold = src[c]->max_threshold;
  }
  const bool bank = src[0]->wavelet == DSX_WAVELET_BANK;
  if (bank && !ctx->wl_set) return fail(ctx, DSX_EINVAL, "DSX_WAVELET_BANK without dsx_set_wavelet");
  if (!ctx->rot_next)
    return plan_chain(ctx, height, width, max_batch, bank, microscope_high_int, flat, dark, dark_h, dark_w);
  // dsx_set_rotate: the chain of np.rot90 of the plane; the shading planes are turned with it
  if (int rc = plan_chain(ctx, width, height, max_batch, bank, microscope_high_int, nullptr, nullptr, 0, 0)) return rc;
  ctx->rot = true;
  ctx->rot_H = height;
  ctx->rot_W = width;
  if (flat)
    if (int rc = rotated_shading_host(ctx, flat, dark, dark_h, dark_w)) { ctx->planned = false; return rc; }
  return DSX_OK;
}

namespace {
// flat [H, W] and dark [dark_h, dark_w] (cropped to [H, W] first) of the caller's orientation as np.rot90 of them:
// [W, H] each, what the epilogue of a rotated plan indexes.
void rotate_shading(const float* flat, const float* dark, int dark_w, int H, int W, std::vector<float>& rflat,
                    std::vector<float>& rdark) {
  const size_t px = (size_t)H * W;
  std::vector<float> crop(px);
  for (int y = 0; y < H; ++y) memcpy(crop.data() + (size_t)y * W, dark + (size_t)y * dark_w, sizeof(float) * W);
  rflat.resize(px);
  rdark.resize(px);
  dsx::rot::rot90_host(flat, rflat.data(), 1, H, W, +1);
  dsx::rot::rot90_host(crop.data(), rdark.data(), 1, H, W, +1);
}

// Shading of a rotated log-space plan from host planes in the caller's orientation: flat [Hout', Wout'] with
// Hout' = plan.Wout, Wout' = plan.Hout (the result plane as the caller sees it), dark at least that.
int rotated_shading_host(dsx_ctx* ctx, const float* flat, const float* dark, int dark_h, int dark_w) {
  const dsx::Plan& p = ctx->plan;
  const int Ho = p.Wout, Wo = p.Hout;
  if (dark_h < Ho || dark_w < Wo) return fail(ctx, DSX_EINVAL, "Please, check the shape of the darkfield.");
  std::vector<float> rflat, rdark;
  rotate_shading(flat, dark, dark_w, Ho, Wo, rflat, rdark);
  const size_t fb = sizeof(float) * (size_t)Ho * Wo;
  DSX_HIP(hipMalloc((void**)&ctx->d_flat, fb));
  DSX_HIP(hipMalloc((void**)&ctx->d_dark, fb));
  ctx->own_shading = true;
  DSX_HIP(hipMemcpy(ctx->d_flat, rflat.data(), fb, hipMemcpyHostToDevice));
  DSX_HIP(hipMemcpy(ctx->d_dark, rdark.data(), fb, hipMemcpyHostToDevice));
  ctx->dark_h = p.Hout;
  ctx->dark_w = p.Wout;
  ctx->workspace_bytes += 2 * fb;
  return DSX_OK;
}

int plan_chain(dsx_ctx* ctx, int height, int width, int max_batch, bool bank, double microscope_high_int,
               const float* flat, const float* dark, int dark_h, int dark_w) {
  ctx->wl_len = bank ? ctx->wl_bank_len : 0;
  if (bank) {
    memcpy(ctx->wl, ctx->wl_bank, sizeof(ctx->wl));
    // the level kernels stage their patches in dynamic LDS: up to 110 KB at 104 taps
    const void* fns[6] = {(const void*)dsx::k_fwd_gen<0>, (const void*)dsx::k_fwd_gen<1>, (const void*)dsx::k_fwd_gen<2>,
                          (const void*)dsx::k_inv_gen<0>, (const void*)dsx::k_inv_gen<1>, (const void*)dsx::k_inv_gen<2>};
    for (const void* fn : fns)
      DSX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dsx::kLdsLimit));
  }
  const std::string perr = dsx::build_plan(height, width, ctx->cfg, ctx->plan, bank ? ctx->wl_bank_len : dsx::kFilterLen);
  if (!perr.empty()) {
    const bool limit = perr.find("too") != std::string::npos;
    return fail(ctx, limit ? DSX_ELIMIT : DSX_EINVAL, perr);
  }
  const dsx::Plan& p = ctx->plan;
  ctx->high_int = microscope_high_int;
  ctx->max_batch = max_batch;
  const int L = p.L, Lc = L > 0 ? L : 1;

  const size_t ws_bytes = (size_t)max_batch * p.plane_floats * sizeof(float);
  DSX_HIP(hipMalloc((void**)&ctx->d_ws, ws_bytes));
  const size_t stats_b = sizeof(dsx::PlaneStats) * max_batch;
  const size_t minmax_b = sizeof(unsigned) * 2 * Lc * max_batch;
  const size_t hist_b = sizeof(unsigned) * 256 * Lc * max_batch;
  ctx->ctl_zero_bytes = stats_b + minmax_b + hist_b;
  DSX_HIP(hipMalloc((void**)&ctx->d_ctl, ctx->ctl_zero_bytes));
  ctx->d_stats = (dsx::PlaneStats*)ctx->d_ctl;
  ctx->d_minmax = (unsigned*)(ctx->d_ctl + stats_b);
  ctx->d_hist = (unsigned*)(ctx->d_ctl + stats_b + minmax_b);
  DSX_HIP(hipMalloc((void**)&ctx->d_thr, sizeof(float) * Lc * max_batch));
  DSX_HIP(hipMalloc((void**)&ctx->d_otsu, sizeof(float) * Lc * max_batch));
  DSX_HIP(hipMalloc((void**)&ctx->d_cfg, sizeof(int) * max_batch));
  DSX_HIP(hipMalloc((void**)&ctx->d_means, sizeof(double) * 2 * max_batch));
  DSX_HIP(hipMemset(ctx->d_cfg, 0, sizeof(int) * max_batch));
  DSX_HIP(hipMemset(ctx->d_means, 0, sizeof(double) * 2 * max_batch));
  DSX_HIP(hipMemset(ctx->d_thr, 0, sizeof(float) * Lc * max_batch));
  DSX_HIP(hipMemset(ctx->d_otsu, 0, sizeof(float) * Lc * max_batch));
  ctx->consts_bytes = std::max<size_t>(p.consts.size(), 1) * sizeof(dsx::C32);
  DSX_HIP(hipMalloc((void**)&ctx->d_consts, ctx->consts_bytes));
  if (!p.consts.empty())
    DSX_HIP(hipMemcpy(ctx->d_consts, p.consts.data(), p.consts.size() * sizeof(dsx::C32), hipMemcpyHostToDevice));
  ctx->workspace_bytes = ws_bytes + ctx->ctl_zero_bytes + ctx->consts_bytes;

  if (flat) {
    if (dark_h < p.Hout || dark_w < p.Wout)
      return fail(ctx, DSX_EINVAL, "Please, check the shape of the darkfield.");
    const size_t fb = sizeof(float) * (size_t)p.Hout * p.Wout;
    const size_t db = sizeof(float) * (size_t)dark_h * dark_w;
    DSX_HIP(hipMalloc((void**)&ctx->d_flat, fb));
    DSX_HIP(hipMalloc((void**)&ctx->d_dark, db));
    ctx->own_shading = true;
    DSX_HIP(hipMemcpy(ctx->d_flat, flat, fb, hipMemcpyHostToDevice));
    DSX_HIP(hipMemcpy(ctx->d_dark, dark, db, hipMemcpyHostToDevice));
    ctx->dark_h = dark_h;
    ctx->dark_w = dark_w;
    ctx->workspace_bytes += fb + db;
  }
  ctx->planned = true;
  ctx->last_n = 0;
  return DSX_OK;
}
}  // namespace

int dsx_set_wavelet(dsx_ctx* ctx, const double* dec_lo, const double* dec_hi, const double* rec_lo,
                    const double* rec_hi, int len) {
  if (!ctx) return DSX_EINVAL;
  if (!dec_lo || !dec_hi || !rec_lo || !rec_hi) return fail(ctx, DSX_EINVAL, "filter pointer is NULL");
  if (len < 2 || (len & 1)) return fail(ctx, DSX_EINVAL, "wavelet filters must have an even number (>= 2) of taps");
  if (len > dsx::kMaxTaps) return fail(ctx, DSX_ELIMIT, "wavelet filters are longer than the kernels take");
  const double* src[4] = {dec_lo, dec_hi, rec_lo, rec_hi};
  for (int f = 0; f < 4; ++f)
    for (int t = 0; t < len; ++t) {
      if (!(fabs(src[f][t]) < 1e30)) return fail(ctx, DSX_EINVAL, "wavelet filter coefficient is not finite");
      ctx->wl_bank[f][t] = (float)src[f][t];
    }
  ctx->wl_bank_len = len;
  ctx->wl_set = true;
  return DSX_OK;  // takes effect at the next dsx_plan whose configs carry DSX_WAVELET_BANK
}

int dsx_set_shading_device(dsx_ctx* ctx, const float* d_flat, const float* d_dark, int dark_h,
                           int dark_w) {
  if (!ctx) return DSX_EINVAL;
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if ((d_flat == nullptr) != (d_dark == nullptr))
    return fail(ctx, DSX_EINVAL, "flatfield and darkfield must be given together");
  const bool rot = ctx->rot && !ctx->streaks;  // the caller's result plane is [plan.Wout, plan.Hout] then
  const int Ho = rot ? ctx->plan.Wout : ctx->plan.Hout, Wo = rot ? ctx->plan.Hout : ctx->plan.Wout;
  if (d_flat && (dark_h < Ho || dark_w < Wo))
    return fail(ctx, DSX_EINVAL, "Please, check the shape of the darkfield.");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  drop_graphs(ctx);  // captured final kernels carry the old shading addresses
  if (ctx->own_shading) { (void)hipFree(ctx->d_flat); (void)hipFree(ctx->d_dark); }
  ctx->own_shading = false;
  if (rot && d_flat) {
    // a rotated plan keeps its own np.rot90 of the planes: the dark is cropped to the plane first, then both are turned
    ctx->d_flat = ctx->d_dark = nullptr;
    const size_t fb = sizeof(float) * (size_t)Ho * Wo;
    float* crop = nullptr;
    DSX_HIP(hipMalloc((void**)&crop, fb));
    hipError_t e = hipMalloc((void**)&ctx->d_flat, fb);
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_dark, fb);
    hipStream_t s = use_main(ctx);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(crop, sizeof(float) * Wo, d_dark, sizeof(float) * dark_w, sizeof(float) * Wo, Ho,
                           hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) {
      rot_planes(s, d_flat, ctx->d_flat, DSX_F32, 1, Ho, Wo, +1);
      rot_planes(s, crop, ctx->d_dark, DSX_F32, 1, Ho, Wo, +1);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(crop);
    if (e != hipSuccess) {
      (void)hipFree(ctx->d_flat); (void)hipFree(ctx->d_dark);
      ctx->d_flat = ctx->d_dark = nullptr;
      return fail(ctx, DSX_EHIP, std::string("rotated shading planes: ") + hipGetErrorString(e));
    }
    ctx->own_shading = true;
    ctx->dark_h = ctx->plan.Hout;
    ctx->dark_w = ctx->plan.Wout;
    return DSX_OK;
  }
  ctx->d_flat = const_cast<float*>(d_flat);
  ctx->d_dark = const_cast<float*>(d_dark);
  ctx->dark_h = dark_h;
  ctx->dark_w = dark_w;
  return DSX_OK;
}

int dsx_graph_stats(const dsx_ctx* ctx, uint64_t* launches, uint64_t* captures) {
  if (!ctx || !launches || !captures) return DSX_EINVAL;
  *launches = ctx->graph_launches;
  *captures = ctx->graph_captures;
  return DSX_OK;
}

int dsx_row_pack_launches(const dsx_ctx* ctx, uint64_t* launches) {
  if (!ctx || !launches) return DSX_EINVAL;
  *launches = ctx->row_pack_launches;
  return DSX_OK;
}

int dsx_constants_device(const dsx_ctx* ctx, void** d_ptr, size_t* bytes) {
  if (!ctx || !ctx->planned || !d_ptr || !bytes) return DSX_EINVAL;
  *d_ptr = ctx->d_consts;
  *bytes = ctx->plan.consts.size() * sizeof(dsx::C32);
  return DSX_OK;
}

int dsx_plan_info(const dsx_ctx* ctx, dsx_plan_info_t* info) {
  if (!ctx || !info) return DSX_EINVAL;
  if (!ctx->planned) return DSX_ENOPLAN;
  memset(info, 0, sizeof(*info));
  const dsx::Plan& p = ctx->plan;
  info->height = p.H; info->width = p.W;
  info->out_height = p.Hout; info->out_width = p.Wout;
  if (ctx->rot) {  // the caller's orientation; the level entries below stay those of the rotated chain
    info->height = p.W; info->width = p.H;
    info->out_height = p.Wout; info->out_width = p.Hout;
  }
  info->levels = p.L;
  for (int l = 0; l < p.L && l < 16; ++l) {
    info->level_h[l] = p.lv[l].h;
    info->level_w[l] = p.lv[l].w;
    info->fft_len[l] = p.lv[l].M;
    info->fft_halo[l] = p.lv[l].K;
  }
  info->max_batch = ctx->max_batch;
  info->workspace_bytes = ctx->workspace_bytes;
  return DSX_OK;
}

int dsx_run_device(dsx_ctx* ctx, const void* d_in, int in_dtype, int n, void* d_out, int out_dtype,
                   int32_t* d_cfg_used) {
  if (!ctx) return DSX_EINVAL;
  if (ctx->streaks) return streaks_run(ctx, d_in, in_dtype, n, d_out, out_dtype, false);
  if (ctx->lightsheet) return lightsheet_run(ctx, d_in, in_dtype, n, d_out, out_dtype, false);
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if (int rc = check_run_args(ctx, d_in, d_out, n, in_dtype, out_dtype)) return rc;
  DSX_HIP(hipSetDevice(ctx->device));
  if (ctx->stack_mode && n > ctx->max_batch)
    return fail(ctx, DSX_ELIMIT, "stack mode: all planes of the stack must fit one cohort (plan with max_batch >= n)");
  const dsx::Plan& p = ctx->plan;
  const size_t in_plane = (size_t)p.H * p.W * elem_size(in_dtype);
  const size_t out_plane = (size_t)p.Hout * p.Wout * elem_size(out_dtype);
  for (int start = 0; start < n; start += ctx->max_batch) {
    const int nb = std::min(ctx->max_batch, n - start);
    const int rc = run_cohort_split(ctx, (const char*)d_in + start * in_plane, in_dtype, nb,
                                    (char*)d_out + start * out_plane, out_dtype,
                                    d_cfg_used ? d_cfg_used + start : nullptr, in_plane, out_plane);
    if (rc != DSX_OK) return rc;
    ctx->last_n = nb;
  }
  return DSX_OK;
}

int dsx_sync(dsx_ctx* ctx) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  return check_sticky(ctx);
}

int dsx_run_host(dsx_ctx* ctx, const void* in, int in_dtype, int n, void* out, int out_dtype,
                 int32_t* cfg_used) {
  if (!ctx) return DSX_EINVAL;
  if (ctx->streaks) return streaks_run(ctx, in, in_dtype, n, out, out_dtype, true);
  if (ctx->lightsheet) return lightsheet_run(ctx, in, in_dtype, n, out, out_dtype, true);
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if (int rc = check_run_args(ctx, in, out, n, in_dtype, out_dtype)) return rc;
  DSX_HIP(hipSetDevice(ctx->device));
  const dsx::Plan& p = ctx->plan;
  const size_t in_plane = (size_t)p.H * p.W * elem_size(in_dtype);
  const size_t out_plane = (size_t)p.Hout * p.Wout * elem_size(out_dtype);
  const int B = ctx->max_batch;
  if (ctx->stack_mode && n > B)
    return fail(ctx, DSX_ELIMIT, "stack mode: all planes of the stack must fit one cohort (plan with max_batch >= n)");
  const size_t need_in = in_plane * B, need_out = out_plane * B + sizeof(int32_t) * B;
  if (int rc = grow_stage(ctx, &ctx->d_stage_in, &ctx->stage_in_bytes, need_in)) return rc;
  if (int rc = grow_stage(ctx, &ctx->d_stage_out, &ctx->stage_out_bytes, need_out)) return rc;
  int32_t* d_cfg = (int32_t*)((char*)ctx->d_stage_out + out_plane * B);
  // A value error of an EARLIER asynchronous dsx_run_device call on this context that nobody has synchronised with yet
  // is reported now (this call synchronises) instead of being wiped by this call's own bookkeeping below.
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  if (int rc = check_sticky(ctx)) return rc;
  for (int start = 0; start < n; start += B) {
    const int nb = std::min(B, n - start);
    DSX_HIP(hipMemcpyAsync(ctx->d_stage_in, (const char*)in + start * in_plane, in_plane * nb,
                           hipMemcpyHostToDevice, use_main(ctx)));
    const int rc = run_cohort_split(ctx, ctx->d_stage_in, in_dtype, nb, ctx->d_stage_out, out_dtype, d_cfg,
                                    in_plane, out_plane);
    if (rc != DSX_OK) return rc;
    ctx->last_n = nb;
    if (ctx->stop_after == 0)
      DSX_HIP(hipMemcpyAsync((char*)out + start * out_plane, ctx->d_stage_out, out_plane * nb,
                             hipMemcpyDeviceToHost, use_main(ctx)));
    if (cfg_used)
      DSX_HIP(hipMemcpyAsync(cfg_used + start, d_cfg, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, use_main(ctx)));
    DSX_HIP(hipStreamSynchronize(use_main(ctx)));
    // float32 planes: the forward kernel flags pixels whose log(1 + x) is not finite (PlaneStats::flags); with at
    // least one decomposition level the reference raises ValueError for such a plane (numpy.histogram inside
    // threshold_otsu: "autodetected range of [nan, nan] is not finite")
    if (p.L > 0) {
      std::vector<dsx::PlaneStats> hs((size_t)nb);
      DSX_HIP(hipMemcpy(hs.data(), ctx->d_stats, sizeof(dsx::PlaneStats) * nb, hipMemcpyDeviceToHost));
      // everything before this call was synchronised and reported above: what the word holds now is this cohort's own,
      // reported right here, per plane
      if (ctx->h_sticky) (void)__atomic_exchange_n(ctx->h_sticky, 0u, __ATOMIC_ACQ_REL);
      for (int k = 0; k < nb && in_dtype == DSX_F32; ++k)
        if (hs[(size_t)k].flags & 1ull)
          return fail(ctx, DSX_EVALUE, "plane " + std::to_string(start + k) +
                                           ": autodetected range of [nan, nan] is not finite (a pixel is NaN, "
                                           "infinite or <= -1)");
    }
  }
  return DSX_OK;
}

/* ---- memory + timing helpers ------------------------------------------------------------------ */
int dsx_malloc(dsx_ctx* ctx, size_t bytes, void** d_ptr) {
  if (!ctx || !d_ptr) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
  if (e != hipSuccess) return fail(ctx, DSX_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return DSX_OK;
}
int dsx_free(dsx_ctx* ctx, void* d_ptr) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  DSX_HIP(hipFree(d_ptr));
  return DSX_OK;
}
int dsx_memcpy_h2d(dsx_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, use_main(ctx)));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  return DSX_OK;
}
int dsx_memcpy_d2h(dsx_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, use_main(ctx)));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  return DSX_OK;
}
int dsx_memcpy_d2d(dsx_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, use_main(ctx)));
  return DSX_OK;
}
/* pinned host memory + copies on their own streams: the overlapped chunk map (zarr_destriper.py) */
namespace {
hipStream_t pick_stream(dsx_ctx* ctx, int id) {
  if (id == DSX_STREAM_UPLOAD) return ctx->copy_stream[0];
  if (id == DSX_STREAM_DOWNLOAD) return ctx->copy_stream[1];
  return use_main(ctx);
}
bool stream_id_ok(int id) { return id == DSX_STREAM_COMPUTE || id == DSX_STREAM_UPLOAD || id == DSX_STREAM_DOWNLOAD; }
}  // namespace
int dsx_malloc_host(dsx_ctx* ctx, size_t bytes, void** h_ptr) {
  if (!ctx || !h_ptr) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  hipError_t e = hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) return fail(ctx, DSX_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  return DSX_OK;
}
int dsx_free_host(dsx_ctx* ctx, void* h_ptr) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipHostFree(h_ptr));
  return DSX_OK;
}
int dsx_memcpy_h2d_async(dsx_ctx* ctx, void* d_dst, const void* src, size_t bytes, int stream_id) {
  if (!ctx || !stream_id_ok(stream_id)) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, pick_stream(ctx, stream_id)));
  return DSX_OK;
}
int dsx_memcpy_d2h_async(dsx_ctx* ctx, void* dst, const void* d_src, size_t bytes, int stream_id) {
  if (!ctx || !stream_id_ok(stream_id)) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, pick_stream(ctx, stream_id)));
  return DSX_OK;
}
int dsx_stream_wait(dsx_ctx* ctx, int waiter, int signaller) {
  if (!ctx || !stream_id_ok(waiter) || !stream_id_ok(signaller)) return DSX_EINVAL;
  if (waiter == signaller) return DSX_OK;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipEventRecord(ctx->ev_xs, pick_stream(ctx, signaller)));
  DSX_HIP(hipStreamWaitEvent(pick_stream(ctx, waiter), ctx->ev_xs, 0));
  return DSX_OK;
}
int dsx_event_record(dsx_ctx* ctx, int slot, int stream_id) {
  if (!ctx || slot < 0 || slot >= dsx_ctx::kEventSlots || !stream_id_ok(stream_id)) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipEventRecord(ctx->ev_slot[slot], pick_stream(ctx, stream_id)));
  return DSX_OK;
}
int dsx_event_sync(dsx_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= dsx_ctx::kEventSlots) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipEventSynchronize(ctx->ev_slot[slot]));
  return check_sticky(ctx);
}
int dsx_stream_sync(dsx_ctx* ctx, int stream_id) {
  if (!ctx || !stream_id_ok(stream_id)) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(pick_stream(ctx, stream_id)));
  return check_sticky(ctx);
}
int dsx_timer_start(dsx_ctx* ctx) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipEventRecord(ctx->t0, use_main(ctx)));
  return DSX_OK;
}
int dsx_timer_stop(dsx_ctx* ctx, float* ms) {
  if (!ctx || !ms) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipEventRecord(ctx->t1, use_main(ctx)));
  DSX_HIP(hipEventSynchronize(ctx->t1));
  DSX_HIP(hipEventElapsedTime(ms, ctx->t0, ctx->t1));
  return DSX_OK;
}
int dsx_profile_enable(dsx_ctx* ctx, int on) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  for (auto& r : ctx->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  ctx->prof.clear();
  ctx->profiling = on != 0;
  return DSX_OK;
}
int dsx_profile_read(dsx_ctx* ctx, int max_classes, float* ms, int32_t* launches, const char** names,
                     int* n_classes) {
  if (!ctx || !ms || !launches || !n_classes) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  const int nc = std::min<int>(max_classes, KC_COUNT);
  for (int i = 0; i < nc; ++i) { ms[i] = 0.f; launches[i] = 0; if (names) names[i] = kClassNames[i]; }
  for (auto& r : ctx->prof) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess && r.cls < nc) { ms[r.cls] += t; launches[r.cls]++; }
  }
  *n_classes = nc;
  return DSX_OK;
}

/* ---- f1 / f3: Zarr brick re-tiling and the 2x2x2 pyramid level (dsx_retile.h) --------------- */
namespace {
int retile_vec(const void* a, const void* b, int W, int cx) {
  int v = 8;
  while (v > 1 && (W % v || cx % v || (uintptr_t)a % (2 * v) || (uintptr_t)b % (2 * v))) v >>= 1;
  return v;
}
int brick_args(dsx_ctx* ctx, dsx::BrickArgs& a, int Z, int H, int W, int cz, int cy, int cx, int z0) {
  if (Z <= 0 || H <= 0 || W <= 0 || cz <= 0 || cy <= 0 || cx <= 0 || z0 < 0)
    return fail(ctx, DSX_EINVAL, "brick re-tiling: shapes must be positive");
  a.Z = Z; a.H = H; a.W = W; a.cz = cz; a.cy = cy; a.cx = cx; a.z0 = z0;
  a.nbz = (z0 + Z + cz - 1) / cz; a.nby = (H + cy - 1) / cy; a.nbx = (W + cx - 1) / cx;
  if ((long long)a.nby * cy > 65535 || (long long)a.nbz * cz > 65535)
    return fail(ctx, DSX_ELIMIT, "brick re-tiling: more than 65535 rows or planes per call");
  return DSX_OK;
}
}  // namespace

int dsx_bricks_to_planes_u16(dsx_ctx* ctx, const void* d_bricks, void* d_planes, int Z, int H, int W, int cz,
                             int cy, int cx, int z0) {
  if (!ctx || !d_bricks || !d_planes) return DSX_EINVAL;
  dsx::BrickArgs a;
  if (int rc = brick_args(ctx, a, Z, H, W, cz, cy, cx, z0)) return rc;
  a.src = (const uint16_t*)d_bricks; a.dst = (uint16_t*)d_planes;
  DSX_HIP(hipSetDevice(ctx->device));
  const int v = retile_vec(d_bricks, d_planes, W, cx);
  const dim3 grid((W / v + 255) / 256, H, Z);
  switch (v) {
    case 8: hipLaunchKernelGGL(dsx::k_bricks_to_planes<8>, grid, dim3(256), 0, use_main(ctx), a); break;
    case 4: hipLaunchKernelGGL(dsx::k_bricks_to_planes<4>, grid, dim3(256), 0, use_main(ctx), a); break;
    case 2: hipLaunchKernelGGL(dsx::k_bricks_to_planes<2>, grid, dim3(256), 0, use_main(ctx), a); break;
    default: hipLaunchKernelGGL(dsx::k_bricks_to_planes<1>, grid, dim3(256), 0, use_main(ctx), a); break;
  }
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_planes_to_bricks_u16(dsx_ctx* ctx, const void* d_planes, void* d_bricks, int Z, int H, int W, int cz,
                             int cy, int cx, int z0) {
  if (!ctx || !d_bricks || !d_planes) return DSX_EINVAL;
  dsx::BrickArgs a;
  if (int rc = brick_args(ctx, a, Z, H, W, cz, cy, cx, z0)) return rc;
  a.src = (const uint16_t*)d_planes; a.dst = (uint16_t*)d_bricks;
  DSX_HIP(hipSetDevice(ctx->device));
  const int v = retile_vec(d_bricks, d_planes, W, cx);
  const dim3 grid((a.nbx * cx / v + 255) / 256, a.nby * cy, a.nbz * cz);
  switch (v) {
    case 8: hipLaunchKernelGGL(dsx::k_planes_to_bricks<8>, grid, dim3(256), 0, use_main(ctx), a); break;
    case 4: hipLaunchKernelGGL(dsx::k_planes_to_bricks<4>, grid, dim3(256), 0, use_main(ctx), a); break;
    case 2: hipLaunchKernelGGL(dsx::k_planes_to_bricks<2>, grid, dim3(256), 0, use_main(ctx), a); break;
    default: hipLaunchKernelGGL(dsx::k_planes_to_bricks<1>, grid, dim3(256), 0, use_main(ctx), a); break;
  }
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_downsample2_u16(dsx_ctx* ctx, const void* d_src, void* d_dst, int Z, int Y, int X) {
  if (!ctx || !d_src || !d_dst) return DSX_EINVAL;
  if (Z < 2 || Y < 2 || X < 2) return fail(ctx, DSX_EINVAL, "downsample: every axis needs at least 2 voxels");
  dsx::DownArgs a;
  a.src = (const uint16_t*)d_src; a.dst = (uint16_t*)d_dst;
  a.Z = Z; a.Y = Y; a.X = X; a.Zo = Z / 2; a.Yo = Y / 2; a.Xo = X / 2;
  if (a.Yo > 65535 || a.Zo > 65535) return fail(ctx, DSX_ELIMIT, "downsample: more than 65535 rows or planes");
  DSX_HIP(hipSetDevice(ctx->device));
  const dim3 grid(((a.Xo + 3) / 4 + 255) / 256, a.Yo, a.Zo);
  const bool vec = X % 8 == 0 && (uintptr_t)d_src % 16 == 0 && (uintptr_t)d_dst % 8 == 0;
  if (vec) hipLaunchKernelGGL(dsx::k_downsample2<true>, grid, dim3(256), 0, use_main(ctx), a);
  else hipLaunchKernelGGL(dsx::k_downsample2<false>, grid, dim3(256), 0, use_main(ctx), a);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

/* ---- histogram of the written volume (dsx_volhist.h): the display window of zarr_destriper.py:722-726 ------------ */
int dsx_volhist_reset(dsx_ctx* ctx) {
  if (!ctx) return DSX_EINVAL;
  DSX_HIP(hipSetDevice(ctx->device));
  if (!ctx->volhist && hipMalloc((void**)&ctx->volhist, (size_t)dsx::vh::kVhBins * 8) != hipSuccess) {
    ctx->volhist = nullptr;
    return fail(ctx, DSX_ENOMEM, "volhist: no device memory for the histogram");
  }
  DSX_HIP(hipMemsetAsync(ctx->volhist, 0, (size_t)dsx::vh::kVhBins * 8, use_main(ctx)));
  return DSX_OK;
}

int dsx_volhist_add_device(dsx_ctx* ctx, const void* d_vox, size_t n) {
  namespace vh = dsx::vh;
  if (!ctx) return DSX_EINVAL;
  if (n == 0) return DSX_OK;
  if (!d_vox) return fail(ctx, DSX_EINVAL, "volhist: the voxel pointer is NULL");
  if ((uintptr_t)d_vox & 1) return fail(ctx, DSX_EINVAL, "volhist: uint16 voxels must be 2-byte aligned");
  if (!ctx->volhist) return fail(ctx, DSX_EINVAL, "volhist: dsx_volhist_reset has not been called");
  if (n >= ((size_t)1 << 32)) return fail(ctx, DSX_ELIMIT, "volhist: 2^32 voxels or more in one call");
  const size_t head = vh::head_voxels(d_vox, n);
  const size_t n_vec = (n - head) / 8, tail = n - head - n_vec * 8;
  const size_t per_block = (size_t)vh::kVhThreads * vh::kVhUnroll;
  const size_t want = std::max<size_t>(1, (n_vec + per_block - 1) / per_block);
  const unsigned grid = (unsigned)std::min<size_t>(want, (size_t)2 * ctx->cus);
  DSX_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(vh::k_volhist_u16, dim3(grid), dim3(vh::kVhThreads), 0, use_main(ctx), (const uint16_t*)d_vox, head,
                     n_vec, tail, ctx->volhist);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_volhist_get(dsx_ctx* ctx, uint64_t* hist) {
  if (!ctx) return DSX_EINVAL;
  if (!hist) return fail(ctx, DSX_EINVAL, "volhist: the result pointer is NULL");
  if (!ctx->volhist) return fail(ctx, DSX_EINVAL, "volhist: dsx_volhist_reset has not been called");
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  DSX_HIP(hipMemcpyAsync(hist, ctx->volhist, (size_t)dsx::vh::kVhBins * 8, hipMemcpyDeviceToHost, s));
  DSX_HIP(hipStreamSynchronize(s));
  return DSX_OK;
}

int dsx_volhist_ref(const void* vox, size_t n, uint64_t* hist) {
  if (n == 0) return DSX_OK;
  if (!vox || !hist) return fail(nullptr, DSX_EINVAL, "volhist: NULL pointer");
  if ((uintptr_t)vox & 1) return fail(nullptr, DSX_EINVAL, "volhist: uint16 voxels must be 2-byte aligned");
  dsx::vh::volhist_host((const uint16_t*)vox, n, hist);
  return DSX_OK;
}

/* ---- per-pixel order statistics of a plane stack (dsx_stackrank.h): the samples of flatfield_estimation.py -------- */
extern "C++" {
namespace {
template <int NQ>
hipError_t launch_stack_rank(const dsx::sr::Geometry& g, int tp_log2, hipStream_t s, const uint16_t* planes, int n, size_t P,
                             unsigned lo, unsigned range, const dsx::sr::Quantiles& qs, uint16_t* out, uint16_t* valid,
                             int vec) {
  namespace sr = dsx::sr;
  if (hipError_t e = raise_lds_limit<sr::k_stack_rank_u16<NQ>>(sr::kSrTileLimit + sr::kSrPartBytes)) return e;
  hipLaunchKernelGGL(sr::k_stack_rank_u16<NQ>, dim3((unsigned)g.grid), dim3(sr::kSrThreads), g.lds_bytes, s, planes, n, P, lo,
                     range, qs, out, valid, tp_log2, vec);
  return hipGetLastError();
}
}  // namespace
}  // extern "C++"

int dsx_stack_rank_u16_device(dsx_ctx* ctx, const void* d_planes, int n, size_t plane_elems, int lo, int hi,
                              const int* q_milli, int n_q, void* d_out, void* d_valid) {
  namespace sr = dsx::sr;
  if (!ctx) return DSX_EINVAL;
  if (const char* why = sr::check_args(d_planes, n, plane_elems, lo, hi, q_milli, n_q, d_out)) return fail(ctx, DSX_EINVAL, why);
  if (((uintptr_t)d_out | (uintptr_t)d_valid) & 1) return fail(ctx, DSX_EINVAL, "stack_rank: uint16 results must be 2-byte aligned");
  const sr::Geometry g = sr::geometry(n, plane_elems);
  const int tp_log2 = g.tp == 256 ? 8 : g.tp == 128 ? 7 : 6;
  const int vec = plane_elems % 8 == 0 && (uintptr_t)d_planes % 16 == 0;
  sr::Quantiles qs = {};
  for (int i = 0; i < n_q; ++i) qs.q[i] = q_milli[i];
  const uint16_t* x = (const uint16_t*)d_planes;
  uint16_t *o = (uint16_t*)d_out, *v = (uint16_t*)d_valid;
  const unsigned ulo = (unsigned)lo, range = (unsigned)(hi - lo);
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  hipError_t e = hipSuccess;
  switch (n_q) {
    case 1: e = launch_stack_rank<1>(g, tp_log2, s, x, n, plane_elems, ulo, range, qs, o, v, vec); break;
    case 2: e = launch_stack_rank<2>(g, tp_log2, s, x, n, plane_elems, ulo, range, qs, o, v, vec); break;
    case 3: e = launch_stack_rank<3>(g, tp_log2, s, x, n, plane_elems, ulo, range, qs, o, v, vec); break;
    default: e = launch_stack_rank<4>(g, tp_log2, s, x, n, plane_elems, ulo, range, qs, o, v, vec); break;
  }
  DSX_HIP(e);
  return DSX_OK;
}

int dsx_stack_rank_u16_ref(const void* planes, int n, size_t plane_elems, int lo, int hi, const int* q_milli, int n_q,
                           void* out, void* valid) {
  namespace sr = dsx::sr;
  if (const char* why = sr::check_args(planes, n, plane_elems, lo, hi, q_milli, n_q, out)) return fail(nullptr, DSX_EINVAL, why);
  if (((uintptr_t)out | (uintptr_t)valid) & 1) return fail(nullptr, DSX_EINVAL, "stack_rank: uint16 results must be 2-byte aligned");
  sr::stack_rank_host((const uint16_t*)planes, n, plane_elems, lo, hi, q_milli, n_q, (uint16_t*)out, (uint16_t*)valid);
  return DSX_OK;
}

/* ---- the finish of a retrospective flat (dsx_smooth.h): fill, Gaussian, mean -- flatfield_estimation.py:15-52 ---------- */
extern "C++" {
namespace {
dsx::sm::Taps smooth_taps(const double* taps, int radius) {
  dsx::sm::Taps t = {};
  for (int k = 0; k <= radius; ++k) t.t[k] = taps[k];
  return t;
}

// The two passes on stream s: in -> tmp along axis 0, tmp -> out along axis 1 (arguments as check_smooth passed them).
hipError_t launch_smooth(hipStream_t s, const double* in, int H, int W, const dsx::sm::Taps& t, int r, double* tmp, double* out) {
  namespace sm = dsx::sm;
  const sm::Geometry g = sm::geometry(H, W, r);
  if (hipError_t e = raise_lds_limit<sm::k_sm_col>(sm::kSmMaxLds)) return e;
  if (hipError_t e = raise_lds_limit<sm::k_sm_row>(sm::kSmMaxLds)) return e;
  const int vec_col = W % 2 == 0 && (uintptr_t)in % 16 == 0, vec_row = W % 2 == 0 && (uintptr_t)tmp % 16 == 0;
  hipLaunchKernelGGL(sm::k_sm_col, dim3(g.col_bx * g.col_by), dim3(sm::kSmThreads), g.col_lds, s, in, tmp, H, W, r, g.col_bx, t,
                     vec_col);
  hipLaunchKernelGGL(sm::k_sm_row, dim3(g.row_bx * g.row_by), dim3(sm::kSmThreads), g.row_lds, s, (const double*)tmp, out, H, W,
                     r, g.row_bx, t, vec_row);
  return hipGetLastError();
}
}  // namespace
}  // extern "C++"

int dsx_gauss_smooth_f64_device(dsx_ctx* ctx, const void* d_in, int H, int W, const double* taps, int radius, void* d_tmp,
                                void* d_out) {
  namespace sm = dsx::sm;
  if (!ctx) return DSX_EINVAL;
  if (const char* why = sm::check_smooth(d_in, H, W, taps, radius, d_tmp, d_out)) return fail(ctx, DSX_EINVAL, why);
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  DSX_HIP(launch_smooth(s, (const double*)d_in, H, W, smooth_taps(taps, radius), radius, (double*)d_tmp, (double*)d_out));
  return DSX_OK;
}

int dsx_gauss_smooth_f64_ref(const void* in, int H, int W, const double* taps, int radius, void* tmp, void* out) {
  namespace sm = dsx::sm;
  if (const char* why = sm::check_smooth(in, H, W, taps, radius, tmp, out)) return fail(nullptr, DSX_EINVAL, why);
  sm::smooth_host((const double*)in, H, W, taps, radius, (double*)tmp, (double*)out);
  return DSX_OK;
}

int dsx_flat_finish_work_bytes(int H, int W, size_t* bytes) {
  namespace sm = dsx::sm;
  if (!bytes || H < 1 || W < 1 || (long long)H * W > sm::kSmMaxElems)
    return fail(nullptr, DSX_EINVAL, "flat_finish_work_bytes: 1 <= H, W and H * W < 2^31");
  *bytes = sm::work_layout(H, W).bytes;
  return DSX_OK;
}

int dsx_flat_finish_device(dsx_ctx* ctx, const void* d_rank, const void* d_valid, int Hs, int Ws, int H, int W, int n_q,
                           const double* taps, int radius, double floor, void* d_flat, void* d_dark, void* d_work) {
  namespace sm = dsx::sm;
  if (!ctx) return DSX_EINVAL;
  if (const char* why = sm::check_finish(d_rank, d_valid, Hs, Ws, H, W, n_q, taps, radius, floor, d_flat, d_dark))
    return fail(ctx, DSX_EINVAL, why);
  if (!d_work || (uintptr_t)d_work % 16) return fail(ctx, DSX_EINVAL, "flat_finish: the work buffer must be 16-byte aligned");
  const sm::Work w = sm::work_layout(H, W);
  char* base = (char*)d_work;
  unsigned* hist = (unsigned*)(base + w.hist);
  sm::Scalars* scal = (sm::Scalars*)(base + w.scal);
  double *part = (double*)(base + w.part), *a = (double*)(base + w.a), *tmp = (double*)(base + w.tmp);
  const sm::Taps t = smooth_taps(taps, radius);
  const int N = H * W;
  const unsigned cover = (unsigned)(((long long)N + sm::kSmThreads - 1) / sm::kSmThreads);
  const unsigned hist_grid = cover < 512u ? cover : 512u;  // two blocks of 64 KiB LDS per CU
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  for (int q = 0; q < n_q; ++q) {
    const uint16_t* R = (const uint16_t*)d_rank + (size_t)q * (size_t)Hs * (size_t)Ws;
    DSX_HIP(hipMemsetAsync(hist, 0, (size_t)sm::kSmBins * sizeof(unsigned), s));
    hipLaunchKernelGGL(sm::k_sm_hist, dim3(hist_grid), dim3(sm::kSmThreads), 0, s, R, (const uint16_t*)d_valid, Ws, W, N, hist);
    hipLaunchKernelGGL(sm::k_sm_median, dim3(1), dim3(sm::kSmThreads), 0, s, (const unsigned*)hist, scal);
    hipLaunchKernelGGL(sm::k_sm_fill, dim3(cover), dim3(sm::kSmThreads), 0, s, R, (const uint16_t*)d_valid, Ws, W, N,
                       (const sm::Scalars*)scal, a);
    DSX_HIP(hipGetLastError());
    DSX_HIP(launch_smooth(s, a, H, W, t, radius, tmp, a));
    if (q == 0) {
      hipLaunchKernelGGL(sm::k_sm_partial, dim3(sm::kSmMeanLanes / sm::kSmThreads), dim3(sm::kSmThreads), 0, s, (const double*)a,
                         N, part);
      hipLaunchKernelGGL(sm::k_sm_mean, dim3(1), dim3(sm::kSmThreads), 0, s, (const double*)part, N, scal);
      hipLaunchKernelGGL(sm::k_sm_norm, dim3(cover), dim3(sm::kSmThreads), 0, s, (const double*)a, N, (const sm::Scalars*)scal,
                         floor, (float*)d_flat);
    } else {
      hipLaunchKernelGGL(sm::k_sm_f32, dim3(cover), dim3(sm::kSmThreads), 0, s, (const double*)a, N, (float*)d_dark);
    }
    DSX_HIP(hipGetLastError());
  }
  unsigned long long seen = 0;  // the one read of the chain: the status
  DSX_HIP(hipMemcpyAsync(&seen, &scal->seen, sizeof(seen), hipMemcpyDeviceToHost, s));
  DSX_HIP(hipStreamSynchronize(s));
  if (!seen) return fail(ctx, DSX_EVALUE, "flat_finish: no pixel of the image is seen (valid is 0 everywhere)");
  return DSX_OK;
}

int dsx_flat_finish_ref(const void* rank, const void* valid, int Hs, int Ws, int H, int W, int n_q, const double* taps,
                        int radius, double floor, void* flat, void* dark) {
  namespace sm = dsx::sm;
  if (const char* why = sm::check_finish(rank, valid, Hs, Ws, H, W, n_q, taps, radius, floor, flat, dark))
    return fail(nullptr, DSX_EINVAL, why);
  if (!sm::flat_finish_host((const uint16_t*)rank, (const uint16_t*)valid, Hs, Ws, H, W, n_q, taps, radius, floor, (float*)flat,
                            (float*)dark))
    return fail(nullptr, DSX_EVALUE, "flat_finish: no pixel of the image is seen (valid is 0 everywhere)");
  return DSX_OK;
}

/* ---- QC projections of the volume a pass reads and writes (dsx_project.h) ------------------------------------------ */
namespace {
// The argument rules both builds share; nullptr when the call may run.
const char* project_args(const void* planes, int Z, int H, int W, const dsx_projection* p, int z_off, int* code) {
  *code = DSX_EINVAL;
  if (Z < 0 || H <= 0 || W <= 0 || z_off < 0) return "project: Z >= 0, H > 0, W > 0 and z_off >= 0";
  if (H > dsx::pj::kPjMaxExtent || W > dsx::pj::kPjMaxExtent || Z > dsx::pj::kPjMaxExtent) {
    *code = DSX_ELIMIT;
    return "project: more than 65536 rows, columns or planes in one call";
  }
  if (Z == 0) return nullptr;
  if (!planes || !p || !p->max_z || !p->sum_z || !p->max_y || !p->sum_y || !p->max_x || !p->sum_x)
    return "project: NULL pointer";
  if ((uintptr_t)planes & 1) return "project: uint16 voxels must be 2-byte aligned";
  return nullptr;
}
}  // namespace

int dsx_project_work_bytes(int Z, int H, int W, size_t* bytes) {
  if (!bytes || Z < 0 || H <= 0 || W <= 0) return DSX_EINVAL;
  if (H > dsx::pj::kPjMaxExtent || W > dsx::pj::kPjMaxExtent || Z > dsx::pj::kPjMaxExtent) return DSX_ELIMIT;
  *bytes = dsx::pj::work_bytes(Z, H, W);
  return DSX_OK;
}

int dsx_project_u16_device(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, const dsx_projection* p, int z_off,
                           int first, void* d_work) {
  namespace pj = dsx::pj;
  if (!ctx) return DSX_EINVAL;
  int code = 0;
  if (const char* e = project_args(d_planes, Z, H, W, p, z_off, &code)) return fail(ctx, code, e);
  if (Z == 0) return DSX_OK;
  if (!d_work) return fail(ctx, DSX_EINVAL, "project: the work buffer is NULL (dsx_project_work_bytes)");
  if ((uintptr_t)d_work & 3) return fail(ctx, DSX_EINVAL, "project: the work buffer must be 4-byte aligned");
  const pj::Partials part = pj::partials(d_work, Z, H, W);
  const int S = pj::strips(W), T = pj::tiles(H);
  const bool vec = W % 8 == 0 && (((uintptr_t)d_planes | (uintptr_t)p->max_z | (uintptr_t)p->sum_z) & 15) == 0;
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  const dim3 grid((unsigned)S, (unsigned)T);
  if (vec)
    hipLaunchKernelGGL(pj::k_project_u16<true>, grid, dim3(pj::kPjThreads), 0, s, (const uint16_t*)d_planes, Z, H, W,
                       p->max_z, (unsigned long long*)p->sum_z, first, part);
  else
    hipLaunchKernelGGL(pj::k_project_u16<false>, grid, dim3(pj::kPjThreads), 0, s, (const uint16_t*)d_planes, Z, H, W,
                       p->max_z, (unsigned long long*)p->sum_z, first, part);
  DSX_HIP(hipGetLastError());
  const size_t n = (size_t)Z * ((size_t)W + H);
  const unsigned fold = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)8 * ctx->cus);
  hipLaunchKernelGGL(pj::k_project_fold, dim3(fold), dim3(256), 0, s, Z, H, W, S, T, part, p->max_y, p->sum_y, p->max_x,
                     p->sum_x, z_off);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_project_u16_ref(const void* planes, int Z, int H, int W, const dsx_projection* p, int z_off, int first) {
  int code = 0;
  if (const char* e = project_args(planes, Z, H, W, p, z_off, &code)) return fail(nullptr, code, e);
  if (Z == 0) return DSX_OK;
  const dsx::pj::Outputs o = {p->max_z, p->sum_z, p->max_y, p->sum_y, p->max_x, p->sum_x};
  dsx::pj::project_host((const uint16_t*)planes, Z, H, W, o, z_off, first != 0);
  return DSX_OK;
}

/* ---- per-chunk content digests of bricks in chunk order (dsx_digest.h): the manifest of a store pass -------------- */
namespace {
const char* digest_args(const void* bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0, int v1, int v2,
                        const void* out) {
  if (const char* e = dsx::dg::check_geometry(n0, n1, n2, c0, c1, c2, v0, v1, v2)) return e;
  if (!bricks || !out) return "digest: NULL pointer";
  if ((uintptr_t)bricks & 1) return "digest: uint16 voxels must be 2-byte aligned";
  if ((uintptr_t)out & 7) return "digest: the records must be 8-byte aligned";
  return nullptr;
}
}  // namespace

int dsx_brick_digest_u16_device(dsx_ctx* ctx, const void* d_bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0,
                                int v1, int v2, void* d_out, int stream_id) {
  namespace dg = dsx::dg;
  if (!ctx) return DSX_EINVAL;
  if (!stream_id_ok(stream_id)) return fail(ctx, DSX_EINVAL, "digest: unknown stream id");
  if (const char* e = digest_args(d_bricks, n0, n1, n2, c0, c1, c2, v0, v1, v2, d_out)) return fail(ctx, DSX_EINVAL, e);
  const int64_t bricks = (int64_t)n0 * n1 * n2;
  const dg::Geometry g = dg::geometry(bricks, c0, c1, c2);
  dg::DigestArgs a;
  a.bricks = (const uint16_t*)d_bricks;
  a.out = (unsigned long long*)d_out;
  a.n1 = n1; a.n2 = n2;
  a.c0 = c0; a.c1 = c1; a.c2 = c2;
  a.v0 = v0; a.v1 = v1; a.v2 = v2;
  a.lx_log2 = 0;
  while ((1 << a.lx_log2) < g.lx) ++a.lx_log2;
  a.segs = (unsigned)g.segs;
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream_id);
  DSX_HIP(hipMemsetAsync(d_out, 0, (size_t)bricks * dg::kDgRecord * 8, s));
  const bool vec = c2 % 8 == 0 && ((uintptr_t)d_bricks & 15) == 0;
  if (vec) hipLaunchKernelGGL(dg::k_brick_digest_u16<true>, dim3((unsigned)g.grid), dim3(dg::kDgThreads), 0, s, a);
  else hipLaunchKernelGGL(dg::k_brick_digest_u16<false>, dim3((unsigned)g.grid), dim3(dg::kDgThreads), 0, s, a);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_brick_digest_u16_ref(const void* bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0, int v1, int v2,
                             void* out) {
  if (const char* e = digest_args(bricks, n0, n1, n2, c0, c1, c2, v0, v1, v2, out)) return fail(nullptr, DSX_EINVAL, e);
  dsx::dg::grid_digest_host((const uint16_t*)bricks, n0, n1, n2, c0, c1, c2, v0, v1, v2, (uint64_t*)out);
  return DSX_OK;
}

/* ---- f3 fused into the chunk map: the pyramid levels of one block (dsx_pyramid.h) ---------------------------- */
namespace {
// Checks the per-level geometry and fills the kernels' view of it; n_out = levels with a non-empty share.
const char* pyramid_levels(int Z, int H, int W, int n_levels, const dsx_pyramid_level* levels, void* const* bricks,
                           dsx::pyr::Level* out, int* n_out, const dsx::pyr::Scale& f = dsx::pyr::Scale{2, 2, 2}) {
  *n_out = 0;
  if (!dsx::pyr::scale_ok(f)) return "pyramid: every scale factor is 1 or 2, and not all are 1";
  if (Z <= 0 || H <= 0 || W <= 0) return "pyramid: the block must not be empty";
  if (n_levels < 1 || n_levels > dsx::pyr::kMaxLevels) return "pyramid: n_levels out of range";
  if (n_levels > 1 && (!levels || !bricks)) return "pyramid: level table is NULL";
  for (int l = 1; l < n_levels; ++l) {
    const dsx_pyramid_level& g = levels[l - 1];
    dsx::pyr::Level& o = out[l - 1];
    o.Z = dsx::pyr::extent(Z, l, f.fz); o.H = dsx::pyr::extent(H, l, f.fy); o.W = dsx::pyr::extent(W, l, f.fx);
    if (o.Z <= 0 || o.H <= 0 || o.W <= 0) break;
    if (!bricks[l - 1]) return "pyramid: brick buffer is NULL";
    if (g.cz <= 0 || g.cy <= 0 || g.cx <= 0 || g.rows <= 0 || g.z0 < 0) return "pyramid: shapes must be positive";
    if ((long long)g.z0 + o.Z > (long long)g.rows * g.cz) return "pyramid: the block's share does not fit the chunk rows";
    o.bricks = (uint16_t*)bricks[l - 1];
    o.cz = g.cz; o.cy = g.cy; o.cx = g.cx; o.z0 = g.z0;
    o.nby = (o.H + g.cy - 1) / g.cy; o.nbx = (o.W + g.cx - 1) / g.cx;
    *n_out = l;
  }
  return nullptr;
}
}  // namespace

int dsx_pyramid_work_bytes(int Z, int H, int W, int n_levels, size_t* bytes) {
  return dsx_pyramid_work_bytes_scale(Z, H, W, 2, 2, 2, n_levels, bytes);
}

int dsx_pyramid_work_bytes_scale(int Z, int H, int W, int fz, int fy, int fx, int n_levels, size_t* bytes) {
  const dsx::pyr::Scale f = {fz, fy, fx};
  if (!bytes || Z < 0 || H < 0 || W < 0 || n_levels < 1 || n_levels > dsx::pyr::kMaxLevels || !dsx::pyr::scale_ok(f))
    return DSX_EINVAL;
  *bytes = dsx::pyr::work_bytes(Z, H, W, n_levels, f);
  return DSX_OK;
}

int dsx_pyramid_block_ref(const void* planes, int Z, int H, int W, int n_levels, const dsx_pyramid_level* levels,
                          void* const* bricks) {
  return dsx_pyramid_block_scale_ref(planes, Z, H, W, 2, 2, 2, n_levels, levels, bricks);
}

int dsx_pyramid_block_scale_ref(const void* planes, int Z, int H, int W, int fz, int fy, int fx, int n_levels,
                                const dsx_pyramid_level* levels, void* const* bricks) {
  if (!planes) return DSX_EINVAL;
  const dsx::pyr::Scale f = {fz, fy, fx};
  dsx::pyr::Level lv[dsx::pyr::kMaxLevels] = {};
  int n = 0;
  if (const char* e = pyramid_levels(Z, H, W, n_levels, levels, bricks, lv, &n, f)) return fail(nullptr, DSX_EINVAL, e);
  for (int l = 1; l <= n; ++l)
    if (levels[l - 1].zero) memset(lv[l - 1].bricks, 0, (size_t)levels[l - 1].rows * dsx::pyr::row_elems(lv[l - 1]) * 2);
  dsx::pyr::pyramid_block_host((const uint16_t*)planes, H, W, n + 1, lv, f);
  return DSX_OK;
}

namespace {
// One level step with a window other than 2 x 2 x 2 (k_pyramid_step): the vector body when every access of a thread is
// whole and aligned, the tail body otherwise.  The caller has checked the scale and the 65535 limits of the grid.
void pyramid_step(const dsx::pyr::Scale& f, bool bricks, hipStream_t s, const dsx::PyrStepArgs& a) {
  const int n = 8 / f.fx;  // output voxels of a thread
  const void* src = bricks ? (const void*)a.bsrc.bricks : (const void*)a.src;
  const bool vec = a.X % 8 == 0 && (uintptr_t)src % 16 == 0 && (!bricks || a.bsrc.cx % 8 == 0) &&
                   (!a.out.bricks || (a.out.cx % n == 0 && (uintptr_t)a.out.bricks % (2 * n) == 0)) &&
                   (uintptr_t)a.dense % (2 * n) == 0;
  const dim3 grid(((a.out.W + n - 1) / n + 255) / 256, a.out.H, a.out.Z);
  switch ((f.fz - 1) * 4 + (f.fy - 1) * 2 + (f.fx - 1)) {
    case 1: dsx::launch_pyramid_step<1, 1, 2>(vec, bricks, grid, s, a); break;
    case 2: dsx::launch_pyramid_step<1, 2, 1>(vec, bricks, grid, s, a); break;
    case 3: dsx::launch_pyramid_step<1, 2, 2>(vec, bricks, grid, s, a); break;
    case 4: dsx::launch_pyramid_step<2, 1, 1>(vec, bricks, grid, s, a); break;
    case 5: dsx::launch_pyramid_step<2, 1, 2>(vec, bricks, grid, s, a); break;
    default: dsx::launch_pyramid_step<2, 2, 1>(vec, bricks, grid, s, a); break;
  }
}

// The levels of a block with a scale other than (2, 2, 2): one step per level, level l from the dense level l - 1 in
// the work buffer (level 1 from the block itself, dense or in chunk order).
int pyramid_run_steps(dsx_ctx* ctx, const void* d_src, const dsx::pyr::BrickSrc* bs, int H, int W, const dsx::pyr::Scale& f,
                      int n, const dsx::pyr::Level* lv, void* d_work, hipStream_t s) {
  uint8_t* work = (uint8_t*)d_work;
  const uint16_t* prev = (const uint16_t*)d_src;
  int Y = H, X = W;
  for (int l = 1; l <= n; ++l) {
    dsx::PyrStepArgs b = {};
    const bool bricks = l == 1 && bs;
    if (bricks) b.bsrc = *bs;
    else b.src = prev;
    b.Y = Y; b.X = X;
    b.out = lv[l - 1];
    b.dense = l < n ? (uint16_t*)work : nullptr;
    pyramid_step(f, bricks, s, b);
    DSX_HIP(hipGetLastError());
    prev = b.dense; Y = b.out.H; X = b.out.W;
    work += ((size_t)b.out.Z * b.out.H * b.out.W * 2 + 15) & ~(size_t)15;
  }
  return DSX_OK;
}

// bs == nullptr: d_src is the dense block (k_pyramid_block); otherwise the block in chunk order (k_pyramid_bricks).
int pyramid_run(dsx_ctx* ctx, const void* d_src, const dsx::pyr::BrickSrc* bs, int Z, int H, int W, int n_levels,
                const dsx_pyramid_level* levels, void* const* d_bricks, void* d_work, size_t work_bytes,
                const dsx::pyr::Scale& f) {
  namespace p = dsx::pyr;
  p::Level lv[p::kMaxLevels] = {};
  int n = 0;
  if (const char* e = pyramid_levels(Z, H, W, n_levels, levels, d_bricks, lv, &n, f)) return fail(ctx, DSX_EINVAL, e);
  if (n == 0) return DSX_OK;
  if (!p::scale_is_2(f)) {
    if (n > 1 && (!d_work || work_bytes < p::work_bytes(Z, H, W, n + 1, f) || (uintptr_t)d_work % 16))
      return fail(ctx, DSX_EINVAL, "pyramid: the work buffer is smaller than dsx_pyramid_work_bytes_scale");
    for (int l = 1; l <= n; ++l)
      if (lv[l - 1].H > 65535 || lv[l - 1].Z > 65535)
        return fail(ctx, DSX_ELIMIT, "pyramid: more than 65535 rows or planes of a level per call");
    DSX_HIP(hipSetDevice(ctx->device));
    hipStream_t s = use_main(ctx);
    for (int l = 1; l <= n; ++l)
      if (levels[l - 1].zero)
        DSX_HIP(hipMemsetAsync(lv[l - 1].bricks, 0, (size_t)levels[l - 1].rows * p::row_elems(lv[l - 1]) * 2, s));
    return pyramid_run_steps(ctx, d_src, bs, H, W, f, n, lv, d_work, s);
  }
  if (n > 2 && (!d_work || work_bytes < p::work_bytes(Z, H, W, n + 1) || (uintptr_t)d_work % 16))
    return fail(ctx, DSX_EINVAL, "pyramid: the work buffer is smaller than dsx_pyramid_work_bytes");
  if ((lv[0].H + 1) / 2 > 65535 || (lv[0].Z + 1) / 2 > 65535)
    return fail(ctx, DSX_ELIMIT, "pyramid: more than 65535 row or plane groups per call");
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  for (int l = 1; l <= n; ++l)
    if (levels[l - 1].zero)
      DSX_HIP(hipMemsetAsync(lv[l - 1].bricks, 0, (size_t)levels[l - 1].rows * p::row_elems(lv[l - 1]) * 2, s));
  p::Level l1 = lv[0], l2 = {};
  if (n >= 2) l2 = lv[1];
  uint8_t* work = (uint8_t*)d_work;
  uint16_t* dense2 = n > 2 ? (uint16_t*)work : nullptr;
  const bool vec = W % 8 == 0 && l1.cx % 4 == 0 && (n < 2 || l2.cx % 2 == 0) && (uintptr_t)d_src % 16 == 0 &&
                   (uintptr_t)l1.bricks % 8 == 0 && (uintptr_t)l2.bricks % 4 == 0;
  const dim3 grid(((l1.W + 3) / 4 + 255) / 256, (l1.H + 1) / 2, (l1.Z + 1) / 2);
  if (bs) {
    dsx::PyrBricksArgs a = {};
    a.src = *bs; a.Z = Z; a.H = H; a.W = W; a.l1 = l1; a.l2 = l2; a.dense2 = dense2;
    if (vec && bs->cx % 8 == 0) hipLaunchKernelGGL(dsx::k_pyramid_bricks<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dsx::k_pyramid_bricks<false>, grid, dim3(256), 0, s, a);
  } else {
    dsx::PyrBlockArgs a = {};
    a.src = (const uint16_t*)d_src; a.Z = Z; a.H = H; a.W = W; a.l1 = l1; a.l2 = l2; a.dense2 = dense2;
    if (vec) hipLaunchKernelGGL(dsx::k_pyramid_block<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dsx::k_pyramid_block<false>, grid, dim3(256), 0, s, a);
  }
  DSX_HIP(hipGetLastError());
  for (int l = 3; l <= n; ++l) {  // dense level l - 1 (in the work buffer) -> level l
    dsx::PyrLevelArgs b = {};
    const p::Level& prev = lv[l - 2];
    b.src = (const uint16_t*)work; b.Y = prev.H; b.X = prev.W;
    work += ((size_t)prev.Z * prev.H * prev.W * 2 + 15) & ~(size_t)15;
    b.out = lv[l - 1];
    b.dense = l < n ? (uint16_t*)work : nullptr;
    const dim3 g((b.out.W + 255) / 256, b.out.H, b.out.Z);
    hipLaunchKernelGGL(dsx::k_pyramid_level, g, dim3(256), 0, s, b);
    DSX_HIP(hipGetLastError());
  }
  return DSX_OK;
}

const char* brick_src(const void* bricks, int H, int W, int cz, int cy, int cx, dsx::pyr::BrickSrc* out) {
  if (cz <= 0 || cy <= 0 || cx <= 0) return "pyramid: the source chunk shape must be positive";
  out->bricks = (const uint16_t*)bricks;
  out->cz = cz; out->cy = cy; out->cx = cx;
  out->nby = (H + cy - 1) / cy; out->nbx = (W + cx - 1) / cx;
  return nullptr;
}
}  // namespace

int dsx_pyramid_block_u16(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, int n_levels,
                          const dsx_pyramid_level* levels, void* const* d_bricks, void* d_work, size_t work_bytes) {
  return dsx_pyramid_block_scale_u16(ctx, d_planes, Z, H, W, 2, 2, 2, n_levels, levels, d_bricks, d_work, work_bytes);
}

int dsx_pyramid_block_scale_u16(dsx_ctx* ctx, const void* d_planes, int Z, int H, int W, int fz, int fy, int fx,
                                int n_levels, const dsx_pyramid_level* levels, void* const* d_bricks, void* d_work,
                                size_t work_bytes) {
  if (!ctx || !d_planes) return DSX_EINVAL;
  return pyramid_run(ctx, d_planes, nullptr, Z, H, W, n_levels, levels, d_bricks, d_work, work_bytes,
                     dsx::pyr::Scale{fz, fy, fx});
}

int dsx_pyramid_bricks_u16(dsx_ctx* ctx, const void* d_src_bricks, int Z, int H, int W, int src_cz, int src_cy,
                           int src_cx, int n_levels, const dsx_pyramid_level* levels, void* const* d_bricks,
                           void* d_work, size_t work_bytes) {
  return dsx_pyramid_bricks_scale_u16(ctx, d_src_bricks, Z, H, W, src_cz, src_cy, src_cx, 2, 2, 2, n_levels, levels,
                                      d_bricks, d_work, work_bytes);
}

int dsx_pyramid_bricks_scale_u16(dsx_ctx* ctx, const void* d_src_bricks, int Z, int H, int W, int src_cz, int src_cy,
                                 int src_cx, int fz, int fy, int fx, int n_levels, const dsx_pyramid_level* levels,
                                 void* const* d_bricks, void* d_work, size_t work_bytes) {
  if (!ctx || !d_src_bricks) return DSX_EINVAL;
  dsx::pyr::BrickSrc bs = {};
  if (const char* e = brick_src(d_src_bricks, H, W, src_cz, src_cy, src_cx, &bs)) return fail(ctx, DSX_EINVAL, e);
  return pyramid_run(ctx, d_src_bricks, &bs, Z, H, W, n_levels, levels, d_bricks, d_work, work_bytes,
                     dsx::pyr::Scale{fz, fy, fx});
}

int dsx_pyramid_bricks_ref(const void* src_bricks, int Z, int H, int W, int src_cz, int src_cy, int src_cx,
                           int n_levels, const dsx_pyramid_level* levels, void* const* bricks) {
  return dsx_pyramid_bricks_scale_ref(src_bricks, Z, H, W, src_cz, src_cy, src_cx, 2, 2, 2, n_levels, levels, bricks);
}

int dsx_pyramid_bricks_scale_ref(const void* src_bricks, int Z, int H, int W, int src_cz, int src_cy, int src_cx, int fz,
                                 int fy, int fx, int n_levels, const dsx_pyramid_level* levels, void* const* bricks) {
  if (!src_bricks) return DSX_EINVAL;
  const dsx::pyr::Scale f = {fz, fy, fx};
  dsx::pyr::BrickSrc bs = {};
  if (const char* e = brick_src(src_bricks, H, W, src_cz, src_cy, src_cx, &bs)) return fail(nullptr, DSX_EINVAL, e);
  dsx::pyr::Level lv[dsx::pyr::kMaxLevels] = {};
  int n = 0;
  if (const char* e = pyramid_levels(Z, H, W, n_levels, levels, bricks, lv, &n, f)) return fail(nullptr, DSX_EINVAL, e);
  for (int l = 1; l <= n; ++l)
    if (levels[l - 1].zero) memset(lv[l - 1].bricks, 0, (size_t)levels[l - 1].rows * dsx::pyr::row_elems(lv[l - 1]) * 2);
  dsx::pyr::pyramid_bricks_host(bs, Z, H, W, n + 1, lv, f);
  return DSX_OK;
}

int dsx_downsample_u16(dsx_ctx* ctx, const void* d_src, void* d_dst, int Z, int Y, int X, int fz, int fy, int fx) {
  namespace p = dsx::pyr;
  const p::Scale f = {fz, fy, fx};
  if (!ctx || !d_src || !d_dst) return DSX_EINVAL;
  if (!p::scale_ok(f)) return fail(ctx, DSX_EINVAL, "downsample: every scale factor is 1 or 2, and not all are 1");
  if (p::scale_is_2(f)) return dsx_downsample2_u16(ctx, d_src, d_dst, Z, Y, X);
  if (Z < fz || Y < fy || X < fx) return fail(ctx, DSX_EINVAL, "downsample: an axis is shorter than its scale factor");
  dsx::PyrStepArgs a = {};
  a.src = (const uint16_t*)d_src; a.Y = Y; a.X = X;
  a.out.Z = Z / fz; a.out.H = Y / fy; a.out.W = X / fx;
  a.dense = (uint16_t*)d_dst;
  if (a.out.H > 65535 || a.out.Z > 65535) return fail(ctx, DSX_ELIMIT, "downsample: more than 65535 rows or planes");
  DSX_HIP(hipSetDevice(ctx->device));
  pyramid_step(f, false, use_main(ctx), a);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_flatfield_correction(dsx_ctx* ctx, const void* d_img, int in_dtype, int H, int W, const float* d_flat,
                             const float* d_dark, int dark_h, int dark_w, float baseline, void* d_out) {
  return dsx_flatfield_correction_rows(ctx, d_img, in_dtype, H, W, d_flat, d_dark, dark_h, dark_w, baseline, nullptr, d_out);
}

int dsx_flatfield_correction_rows(dsx_ctx* ctx, const void* d_img, int in_dtype, int H, int W, const float* d_flat,
                                  const float* d_dark, int dark_h, int dark_w, float baseline,
                                  const float* d_baseline_rows, void* d_out) {
  if (!ctx || !d_img || !d_flat || !d_dark || !d_out) return DSX_EINVAL;
  if (in_dtype != DSX_U16 && in_dtype != DSX_F32) return fail(ctx, DSX_EINVAL, "unknown element type");
  if (H <= 0 || W <= 0 || H > 65535) return fail(ctx, DSX_EINVAL, "flatfield_correction: bad plane shape");
  if (dark_h < H || dark_w < W)
    return fail(ctx, DSX_EINVAL, "Please, check the shape of the darkfield (smaller than the image)");
  dsx::ShadeArgs a;
  a.src = d_img; a.flat = d_flat; a.dark = d_dark; a.dst = (uint16_t*)d_out;
  a.H = H; a.W = W; a.dark_w = dark_w; a.baseline = baseline;
  a.baseline_rows = d_baseline_rows;
  DSX_HIP(hipSetDevice(ctx->device));
  const dim3 grid((W + 255) / 256, H);
  if (in_dtype == DSX_U16) hipLaunchKernelGGL(dsx::k_shade<true>, grid, dim3(256), 0, use_main(ctx), a);
  else hipLaunchKernelGGL(dsx::k_shade<false>, grid, dim3(256), 0, use_main(ctx), a);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_foreground_background(dsx_ctx* ctx, const void* d_img, int in_dtype, size_t n, float cutoff,
                              double* fore_mean, double* back_mean, void* d_mask) {
  if (!ctx || !d_img || !fore_mean || !back_mean) return DSX_EINVAL;
  if (in_dtype != DSX_U16 && in_dtype != DSX_F32) return fail(ctx, DSX_EINVAL, "unknown element type");
  if (n == 0) return fail(ctx, DSX_EINVAL, "empty image");
  DSX_HIP(hipSetDevice(ctx->device));
  char* d_acc = nullptr;
  DSX_HIP(hipMalloc(&d_acc, 32));
  int rc = DSX_OK;
  do {
    if (hipMemsetAsync(d_acc, 0, 32, use_main(ctx)) != hipSuccess) { rc = DSX_EHIP; break; }
    dsx::FgBgArgs a;
    a.src = d_img; a.mask = (uint8_t*)d_mask; a.acc = (double*)d_acc; a.cnt = (unsigned long long*)(d_acc + 16);
    a.n = n; a.cutoff = cutoff;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    if (in_dtype == DSX_U16) hipLaunchKernelGGL(dsx::k_fgbg<true>, dim3(blocks), dim3(256), 0, use_main(ctx), a);
    else hipLaunchKernelGGL(dsx::k_fgbg<false>, dim3(blocks), dim3(256), 0, use_main(ctx), a);
    char h[32];
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h, d_acc, 32, hipMemcpyDeviceToHost, use_main(ctx)) != hipSuccess ||
        hipStreamSynchronize(use_main(ctx)) != hipSuccess) { rc = DSX_EHIP; break; }
    const double* acc = (const double*)h;
    const unsigned long long* cnt = (const unsigned long long*)(h + 16);
    // an empty class has mean 0.0 (filtering.py:84-85)
    *fore_mean = cnt[0] ? acc[0] / (double)cnt[0] : 0.0;
    *back_mean = cnt[1] ? acc[1] / (double)cnt[1] : 0.0;
  } while (0);
  (void)hipFree(d_acc);
  if (rc != DSX_OK) return fail(ctx, rc, "foreground / background statistic failed");
  return DSX_OK;
}


/* ---- multi-GPU: RCCL communicator (one process per GPU) ------------------ */
namespace {
struct RcclApi {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclBroadcast) broadcast = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};
RcclApi g_rccl;

// librccl.so is loaded on first use only: single-GPU users of the library never pay for it.
int load_rccl(dsx_ctx* ctx) {
  if (ctx->rccl) return DSX_OK;
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(ctx, DSX_EHIP, std::string("dlopen(librccl.so): ") + dlerror());
#define DSX_SYM(field, name)                                                            \
  g_rccl.field = (decltype(g_rccl.field))dlsym(h, name);                                \
  if (!g_rccl.field) return fail(ctx, DSX_EHIP, std::string("librccl.so lacks ") + name)
  DSX_SYM(get_unique_id, "ncclGetUniqueId");
  DSX_SYM(comm_init_rank, "ncclCommInitRank");
  DSX_SYM(comm_destroy, "ncclCommDestroy");
  DSX_SYM(broadcast, "ncclBroadcast");
  DSX_SYM(all_reduce, "ncclAllReduce");
  DSX_SYM(error_string, "ncclGetErrorString");
#undef DSX_SYM
  ctx->rccl = h;
  return DSX_OK;
}

#define DSX_NCCL(call)                                                                          \
  do {                                                                                          \
    ncclResult_t r_ = (call);                                                                   \
    if (r_ != ncclSuccess)                                                                      \
      return fail(ctx, DSX_ECOMM, std::string(#call) + ": " + g_rccl.error_string(r_));         \
  } while (0)
}  // namespace

int dsx_comm_unique_id(dsx_ctx* ctx, char* id, size_t id_bytes) {
  if (!ctx || !id) return DSX_EINVAL;
  if (id_bytes < DSX_COMM_ID_BYTES) return fail(ctx, DSX_EINVAL, "unique id buffer too small");
  static_assert(DSX_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  if (int rc = load_rccl(ctx)) return rc;
  DSX_HIP(hipSetDevice(ctx->device));
  ncclUniqueId u;
  DSX_NCCL(g_rccl.get_unique_id(&u));
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return DSX_OK;
}

int dsx_comm_init(dsx_ctx* ctx, const char* id, size_t id_bytes, int rank, int world) {
  if (!ctx || !id) return DSX_EINVAL;
  if (id_bytes < DSX_COMM_ID_BYTES || world < 1 || rank < 0 || rank >= world)
    return fail(ctx, DSX_EINVAL, "bad unique id / rank / world size");
  if (ctx->comm) return fail(ctx, DSX_EINVAL, "communicator already initialised");
  if (int rc = load_rccl(ctx)) return rc;
  DSX_HIP(hipSetDevice(ctx->device));
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  DSX_NCCL(g_rccl.comm_init_rank(&ctx->comm, world, u, rank));
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  DSX_HIP(hipMalloc((void**)&ctx->d_red, sizeof(double) * 64));
  return DSX_OK;
}

int dsx_comm_destroy(dsx_ctx* ctx) {
  if (!ctx) return DSX_EINVAL;
  if (ctx->comm) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(use_main(ctx));
    (void)g_rccl.comm_destroy(ctx->comm);
    ctx->comm = nullptr;
  }
  if (ctx->d_red) { (void)hipFree(ctx->d_red); ctx->d_red = nullptr; }
  ctx->comm_rank = 0;
  ctx->comm_world = 1;
  return DSX_OK;
}

int dsx_comm_broadcast(dsx_ctx* ctx, void* d_buf, size_t bytes, int root) {
  if (!ctx || (!d_buf && bytes)) return DSX_EINVAL;
  if (!ctx->comm) return fail(ctx, DSX_ECOMM, "dsx_comm_init has not been called");
  if (root < 0 || root >= ctx->comm_world) return fail(ctx, DSX_EINVAL, "root out of range");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_NCCL(g_rccl.broadcast(d_buf, d_buf, bytes, ncclUint8, root, ctx->comm, use_main(ctx)));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  return DSX_OK;
}

int dsx_comm_allreduce_f64(dsx_ctx* ctx, double* values, int n, int op) {
  if (!ctx || !values || n < 1 || n > 64) return DSX_EINVAL;
  if (!ctx->comm) return fail(ctx, DSX_ECOMM, "dsx_comm_init has not been called");
  const ncclRedOp_t ops[3] = {ncclSum, ncclMax, ncclMin};
  if (op < 0 || op > 2) return fail(ctx, DSX_EINVAL, "reduction: 0 sum, 1 max, 2 min");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipMemcpyAsync(ctx->d_red, values, sizeof(double) * n, hipMemcpyHostToDevice, use_main(ctx)));
  DSX_NCCL(g_rccl.all_reduce(ctx->d_red, ctx->d_red, n, ncclDouble, ops[op], ctx->comm, use_main(ctx)));
  DSX_HIP(hipMemcpyAsync(values, ctx->d_red, sizeof(double) * n, hipMemcpyDeviceToHost, use_main(ctx)));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  return DSX_OK;
}

/* ---- chunk files <-> staging memory on native threads (dsx_io.h) -------------------------------- */
int dsx_io_read_chunks(dsx_ctx* ctx, const char* const* paths, void* const* dst, const size_t* bytes, int n,
                       int threads, int codec, uint16_t fill_value) {
  if (n < 0 || (n > 0 && (!paths || !dst || !bytes))) return DSX_EINVAL;
  if (codec < DSX_CODEC_RAW || codec > DSX_CODEC_BLOSC) return fail(ctx, DSX_EINVAL, "unknown chunk codec");
  const std::string e = dsx::io_read_chunks(paths, dst, bytes, n, threads, codec, fill_value);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}
int dsx_io_write_chunks(dsx_ctx* ctx, const char* const* paths, const void* const* src, const size_t* bytes, int n,
                        int threads, int zlib_level) {
  if (n < 0 || (n > 0 && (!paths || !src || !bytes))) return DSX_EINVAL;
  const std::string e = dsx::io_write_chunks(paths, src, bytes, n, threads, zlib_level);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}

int dsx_io_write_chunks_blosc(dsx_ctx* ctx, const char* const* paths, const void* const* src, const size_t* bytes,
                              int n, int threads, int clevel, int typesize, int shuffle) {
  if (n < 0 || (n > 0 && (!paths || !src || !bytes))) return DSX_EINVAL;
  if (typesize < 1 || typesize > 255 || clevel < 0 || clevel > 9) return fail(ctx, DSX_EINVAL, "bad Blosc parameters");
  const std::string e = dsx::io_write_chunks(paths, src, bytes, n, threads, clevel, typesize, shuffle != 0);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}
int dsx_blosc_decode(const void* frame, size_t frame_bytes, void* dst, size_t dst_bytes) {
  if (!frame || (!dst && dst_bytes)) return DSX_EINVAL;
  const std::string e = dsx::blosc_decode((const unsigned char*)frame, frame_bytes, dst, dst_bytes);
  if (!e.empty()) return fail(nullptr, DSX_EIO, e);
  return DSX_OK;
}
int dsx_blosc_encode(const void* src, size_t bytes, int typesize, int clevel, int shuffle, void* frame,
                     size_t frame_capacity, size_t* frame_bytes) {
  if ((!src && bytes) || !frame || !frame_bytes) return DSX_EINVAL;
  if (typesize < 1 || typesize > 255 || clevel < 0 || clevel > 9) return fail(nullptr, DSX_EINVAL, "bad Blosc parameters");
  std::vector<unsigned char> out;
  const std::string e = dsx::blosc_encode(src, bytes, typesize, clevel, shuffle != 0, out);
  if (!e.empty()) return fail(nullptr, DSX_EIO, e);
  if (out.size() > frame_capacity) return fail(nullptr, DSX_EINVAL, "frame buffer too small (bytes + 16 always fits)");
  memcpy(frame, out.data(), out.size());
  *frame_bytes = out.size();
  return DSX_OK;
}
int dsx_blosc_encode_lz4(const void* src, size_t bytes, int clevel, void* frame, size_t frame_capacity,
                         size_t* frame_bytes) {
  if ((!src && bytes) || !frame || !frame_bytes) return DSX_EINVAL;
  if (bytes % 2 || clevel < 0 || clevel > 9) return fail(nullptr, DSX_EINVAL, "bad Blosc-LZ4 parameters (uint16 elements)");
  const std::string e = dsx::blosc_encode_lz4(src, bytes, clevel, [&](const unsigned char* f, size_t n) {
    if (n > frame_capacity) return false;
    memcpy(frame, f, n);
    *frame_bytes = n;
    return true;
  });
  if (!e.empty()) return fail(nullptr, DSX_EINVAL, e == "sink" ? "frame buffer too small (bytes + 16 always fits)" : e);
  return DSX_OK;
}
int dsx_io_write_chunks_blosc_lz4(dsx_ctx* ctx, const char* const* paths, const void* const* src, const size_t* bytes,
                                  int n, int threads, int clevel) {
  if (n < 0 || (n > 0 && (!paths || !src || !bytes))) return DSX_EINVAL;
  if (clevel < 0 || clevel > 9) return fail(ctx, DSX_EINVAL, "bad Blosc parameters");
  const std::string e = dsx::io_write_chunks_blosc_lz4(paths, src, bytes, n, threads, clevel);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}

namespace {
const char* zenc_params(int n_chunks, size_t chunk_bytes, int typesize, int clevel, int mode) {
  if (mode != DSX_ZENC_LITERALS && mode != DSX_ZENC_RUNS && mode != DSX_ZENC_LZ4) return "blosc_encode: unknown mode";
  if (typesize != 2) return "blosc_encode: the zstd and LZ4 encoders support typesize 2 only";
  if (n_chunks < 0 || chunk_bytes % 2 || clevel < 0 || clevel > 9) return "blosc_encode: bad parameters";
  if (chunk_bytes > 0x7FFFFFEFu) return "blosc_encode: chunk larger than a frame can hold";
  return nullptr;
}
}  // namespace

int dsx_blosc_encode_ref_ex(const void* src, int n_chunks, size_t chunk_bytes, int typesize, int clevel, void* frames,
                            int64_t* offsets, int mode) {
  if ((!src && n_chunks > 0 && chunk_bytes) || !frames || !offsets) return DSX_EINVAL;
  if (const char* e = zenc_params(n_chunks, chunk_bytes, typesize, clevel, mode)) return fail(nullptr, DSX_EINVAL, e);
  const uint16_t* e = (const uint16_t*)src;
  if (mode == DSX_ZENC_LZ4)  // (either is blosc::assemble_chunks_host over the mode's block encoder)
    dsx::lz4enc::blosc_encode_host(e, (uint64_t)n_chunks, chunk_bytes, clevel, (uint8_t*)frames, offsets);
  else
    dsx::zenc::blosc_encode_host(e, (uint64_t)n_chunks, chunk_bytes, clevel, (uint8_t*)frames, offsets, mode);
  return DSX_OK;
}
int dsx_blosc_encode_ref(const void* src, int n_chunks, size_t chunk_bytes, int typesize, int clevel, void* frames,
                         int64_t* offsets) {
  return dsx_blosc_encode_ref_ex(src, n_chunks, chunk_bytes, typesize, clevel, frames, offsets, DSX_ZENC_LITERALS);
}

int dsx_blosc_encode_device(dsx_ctx* ctx, const void* d_src, int n_chunks, size_t chunk_bytes, int typesize,
                            int clevel, void* d_frames, int64_t* d_offsets) {
  return dsx_blosc_encode_device_ex(ctx, d_src, n_chunks, chunk_bytes, typesize, clevel, d_frames, d_offsets,
                                    DSX_ZENC_LITERALS);
}
int dsx_blosc_encode_device_ex(dsx_ctx* ctx, const void* d_src, int n_chunks, size_t chunk_bytes, int typesize,
                               int clevel, void* d_frames, int64_t* d_offsets, int mode) {
  if (!ctx || (!d_src && n_chunks > 0 && chunk_bytes) || !d_frames || !d_offsets) return DSX_EINVAL;
  if (const char* e = zenc_params(n_chunks, chunk_bytes, typesize, clevel, mode)) return fail(ctx, DSX_EINVAL, e);
  namespace z = dsx::zenc;
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  const bool store = chunk_bytes < (size_t)z::kBloscMinBuffer || clevel == 0;
  const z::Geometry g(chunk_bytes ? chunk_bytes : 1);
  const size_t nblocks = store ? 0 : (size_t)n_chunks * g.nblocks * z::kZPerBlosc;
  if ((size_t)n_chunks * g.nblocks > 0x7FFFFFFFu / z::kZPerBlosc)
    return fail(ctx, DSX_ELIMIT, "blosc_encode: too many blocks per call");
  const char* nomem = "blosc_encode: cannot allocate the work buffer";
  const size_t slot_bytes = nblocks * (size_t)z::kSlotStride, lit_bytes = mode == DSX_ZENC_RUNS ? slot_bytes : 0;
  if (int rc = grow_device(ctx, s, &ctx->zenc_slots, &ctx->zenc_slot_bytes, slot_bytes, nomem)) return rc;
  if (int rc = grow_device(ctx, s, &ctx->zenc_sizes, &ctx->zenc_size_bytes, nblocks * sizeof(uint32_t), nomem)) return rc;
  if (int rc = grow_device(ctx, s, &ctx->zenc_lits, &ctx->zenc_lit_bytes, lit_bytes, nomem)) return rc;
  const z::EncArgs ea{(const uint16_t*)d_src, ctx->zenc_slots, ctx->zenc_sizes, (uint64_t)chunk_bytes, g.nblocks};
  if (nblocks) {  // one workgroup per slot: a zstd block, or (one wave) an LZ4 stream
    if (mode == DSX_ZENC_LZ4)
      hipLaunchKernelGGL(dsx::lz4enc::k_lz4_stream, dim3((unsigned)nblocks), dim3(64), 0, s, ea);
    else if (mode == DSX_ZENC_RUNS)
      hipLaunchKernelGGL(z::k_zenc_block_runs, dim3((unsigned)nblocks), dim3(z::kEncThreads), 0, s,
                         z::RunArgs{ea, ctx->zenc_lits});
    else
      hipLaunchKernelGGL(z::k_zenc_block, dim3((unsigned)nblocks), dim3(z::kEncThreads), 0, s, ea);
  }
  const z::PackArgs pa{(const uint16_t*)d_src, ctx->zenc_slots, ctx->zenc_sizes, (uint8_t*)d_frames, d_offsets,
                       (uint64_t)chunk_bytes, n_chunks, store ? 1 : g.nblocks, store};
  if (mode == DSX_ZENC_LZ4) launch_pack<dsx::lz4enc::Lz4Streams>(s, pa);
  else launch_pack<z::ZstdFrames>(s, pa);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_io_read_frames_ex(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                          uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                          size_t* packed_bytes, int* n_tasks, uint8_t* routes, int mode) {
  if (n < 0 || (n > 0 && (!paths || !packed || !tasks)) || !packed_bytes || !n_tasks || task_capacity < 0)
    return DSX_EINVAL;
  if (mode != DSX_ZDEC_ZSTD && mode != DSX_ZDEC_ANY && mode != DSX_ZDEC_ALL) return DSX_EINVAL;
  const std::string e = dsx::io_read_frames(paths, n, chunk_bytes, threads, fill_value, (unsigned char*)packed,
                                            packed_capacity, (dsx::zdec::DecTask*)tasks, (size_t)task_capacity,
                                            packed_bytes, n_tasks, routes, mode);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}

int dsx_io_read_frames(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                       uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                       size_t* packed_bytes, int* n_tasks, uint8_t* routes) {
  return dsx_io_read_frames_ex(ctx, paths, n, chunk_bytes, threads, fill_value, packed, packed_capacity, tasks,
                               task_capacity, packed_bytes, n_tasks, routes, DSX_ZDEC_ZSTD);
}

int dsx_io_read_zlib_chunks(dsx_ctx* ctx, const char* const* paths, int n, size_t chunk_bytes, int threads,
                            uint16_t fill_value, void* packed, size_t packed_capacity, void* tasks, int task_capacity,
                            size_t* packed_bytes, int* n_tasks, uint8_t* routes) {
  if (n < 0 || (n > 0 && (!paths || !packed || !tasks)) || !packed_bytes || !n_tasks || task_capacity < 0)
    return DSX_EINVAL;
  const std::string e = dsx::io_read_zlib_chunks(paths, n, chunk_bytes, threads, fill_value, (unsigned char*)packed,
                                                 packed_capacity, (dsx::zdec::DecTask*)tasks, (size_t)task_capacity,
                                                 packed_bytes, n_tasks, routes);
  if (!e.empty()) return fail(ctx, DSX_EIO, e);
  return DSX_OK;
}

int dsx_blosc_decode_ref(const void* packed, size_t packed_bytes, const void* tasks, int n_tasks, void* out,
                         size_t out_bytes, int32_t* status) {
  if ((!packed && packed_bytes) || (!tasks && n_tasks) || n_tasks < 0 || (!out && out_bytes) || (!status && n_tasks))
    return DSX_EINVAL;
  namespace z = dsx::zdec;
  const z::DecTask* t = (const z::DecTask*)tasks;
  z::DecWork* work = new z::DecWork;
  std::vector<uint8_t> tmp;
  for (int i = 0; i < n_tasks; ++i) {
    const z::DecTask& k = t[i];
    if (k.dst > out_bytes || k.dst_len > out_bytes - k.dst ||
        ((k.kind & z::kTaskKindMask) != z::kTaskFill && (k.src > packed_bytes || k.src_len > packed_bytes - k.src))) {
      status[i] = z::kErrOutput;
      continue;
    }
    tmp.resize(k.dst_len);
    status[i] = z::run_task_host(*work, k, (const uint8_t*)packed, (uint8_t*)out, tmp.data());
  }
  delete work;
  return DSX_OK;
}

int dsx_blosc_decode_device(dsx_ctx* ctx, const void* d_packed, size_t packed_bytes, const void* d_tasks, int n_tasks,
                            void* d_out, size_t out_bytes, int32_t* d_status) {
  if (!ctx || n_tasks < 0 || (n_tasks > 0 && (!d_packed || !d_tasks || !d_out || !d_status))) return DSX_EINVAL;
  namespace z = dsx::zdec;
  DSX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = use_main(ctx);
  if (int rc = grow_device(ctx, s, &ctx->zdec_scratch, &ctx->zdec_bytes, out_bytes,
                           "blosc_decode: cannot allocate the work buffer"))
    return rc;
  if (n_tasks > 0) {
    const z::DecArgs da{(const uint8_t*)d_packed, (const z::DecTask*)d_tasks, (uint8_t*)d_out,
                        ctx->zdec_scratch, d_status, (uint64_t)packed_bytes, (uint64_t)out_bytes};
    hipLaunchKernelGGL(z::k_zdec, dim3((unsigned)n_tasks), dim3(z::kDecThreads), 0, s, da);
    // the zlib and blosclz tasks (DSX_ZDEC_ALL); the table is on the device, so the launch does not know whether it
    // holds any: a wave of either kernel leaves at once when the task is the other's
    hipLaunchKernelGGL(z::k_zdec_all, dim3((unsigned)n_tasks), dim3(z::kDecThreads), 0, s, da);
  }
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_png_unfilter(void* rows, int height, int stride, int bytes_per_pixel) {
  if (!rows && height > 0) return DSX_EINVAL;
  const std::string e = dsx::png_unfilter((unsigned char*)rows, height, stride, bytes_per_pixel);
  if (!e.empty()) return fail(nullptr, DSX_EIO, e);
  return DSX_OK;
}

/* ---- debug hooks ---------------------------------------------------------------------------- */
int dsx_set_stack_mode(dsx_ctx* ctx, int on) {
  if (!ctx) return DSX_EINVAL;
  const bool want = on != 0;
  // the mode is baked into captured launch chains (Fwd1Args / HistArgs / OtsuArgs::shared) and is not part of the
  // graph cache's key: a graph captured under the other mode must not be replayed
  if (want != ctx->stack_mode) drop_graphs(ctx);
  ctx->stack_mode = want;
  return DSX_OK;
}
int dsx_set_stop_after(dsx_ctx* ctx, int stage) {
  if (!ctx || stage < 0 || stage > 2) return DSX_EINVAL;
  ctx->stop_after = stage;
  return DSX_OK;
}
int dsx_get_stats(dsx_ctx* ctx, int plane, double* fore_mean, double* back_mean, int32_t* cfg_used) {
  if (!ctx) return DSX_EINVAL;
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if (plane < 0 || plane >= ctx->last_n) return fail(ctx, DSX_EINVAL, "plane index outside the last cohort");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  if (int rc = check_sticky(ctx)) return rc;
  double m[2];
  int c = 0;
  DSX_HIP(hipMemcpy(m, ctx->d_means + 2 * plane, sizeof(m), hipMemcpyDeviceToHost));
  DSX_HIP(hipMemcpy(&c, ctx->d_cfg + plane, sizeof(int), hipMemcpyDeviceToHost));
  if (fore_mean) *fore_mean = m[0];
  if (back_mean) *back_mean = m[1];
  if (cfg_used) *cfg_used = c;
  return DSX_OK;
}
int dsx_get_thresholds(dsx_ctx* ctx, int plane, int level, float* otsu, float* threshold) {
  if (!ctx) return DSX_EINVAL;
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if (plane < 0 || plane >= ctx->last_n || level < 0 || level >= ctx->plan.L)
    return fail(ctx, DSX_EINVAL, "plane / level index out of range");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  const size_t i = (size_t)plane * ctx->plan.L + level;
  if (otsu) DSX_HIP(hipMemcpy(otsu, ctx->d_otsu + i, sizeof(float), hipMemcpyDeviceToHost));
  if (threshold) DSX_HIP(hipMemcpy(threshold, ctx->d_thr + i, sizeof(float), hipMemcpyDeviceToHost));
  return DSX_OK;
}
int dsx_get_level(dsx_ctx* ctx, int plane, int level, int stage, float* out) {
  if (!ctx || !out) return DSX_EINVAL;
  if (!ctx->planned) return fail(ctx, DSX_ENOPLAN, "dsx_plan has not been called");
  if (plane < 0 || plane >= ctx->last_n || level < 0 || level >= ctx->plan.L)
    return fail(ctx, DSX_EINVAL, "plane / level index out of range");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  const dsx::LevelPlan& lp = ctx->plan.lv[level];
  const long long off = (stage == DSX_STAGE_APPROX) ? lp.aa_off : lp.da_off;
  const int pitch = (stage == DSX_STAGE_APPROX) ? lp.lda : lp.ld;
  const float* src = ctx->d_ws + (size_t)plane * ctx->plan.plane_floats + off;
  DSX_HIP(hipMemcpy2D(out, sizeof(float) * lp.w, src, sizeof(float) * pitch, sizeof(float) * lp.w, lp.h,
                      hipMemcpyDeviceToHost));
  return DSX_OK;
}

int dsx_plan_streaks(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_streaks_cfg* cfg) {
  return dsx_plan_streaks_ex(ctx, height, width, max_batch, cfg, DSX_STREAKS_GENERIC);
}

int dsx_plan_streaks_ex(dsx_ctx* ctx, int height, int width, int max_batch, const dsx_streaks_cfg* cfg, int route) {
  return dsx_plan_streaks_opts(ctx, height, width, max_batch, cfg, route, nullptr);
}

int dsx_plan_streaks_opts(dsx_ctx* ctx, int height_in, int width_in, int max_batch, const dsx_streaks_cfg* cfg_in,
                          int route, const dsx_streaks_opts* opts) {
  if (!ctx) return DSX_EINVAL;
  // dsx_set_rotate: everything below plans np.rot90 of the caller's plane, [width_in, height_in]
  const bool rot = ctx->rot_next;
  const int height = rot ? width_in : height_in, width = rot ? height_in : width_in;
  const bool has_opts = opts && (opts->bands != DSX_STREAKS_BANDS_BOTH || opts->smoothing != 0.f || opts->flat || opts->dark);
  int clip = 0;
  dsx_streaks_cfg one_sided;
  const dsx_streaks_cfg* cfg = cfg_in;
  if (has_opts) {
    if (opts->bands != DSX_STREAKS_BANDS_BOTH && opts->bands != DSX_STREAKS_BANDS_FG && opts->bands != DSX_STREAKS_BANDS_BG)
      return fail(ctx, DSX_EINVAL, "unknown streaks band choice");
    if (!(opts->smoothing >= 0.f && opts->smoothing <= 2.f))
      return fail(ctx, DSX_EINVAL, "smoothing must be 0 or a value in (0, 2]");
    if ((opts->flat == nullptr) != (opts->dark == nullptr))
      return fail(ctx, DSX_EINVAL, "flatfield and darkfield must be given together");
    if (opts->flat && (opts->dark_h < height_in || opts->dark_w < width_in))
      return fail(ctx, DSX_EINVAL, "Please, check the shape of the darkfield.");
    if (max_batch > 65535) return fail(ctx, DSX_EINVAL, "max_batch too large");
    if (cfg_in && opts->bands != DSX_STREAKS_BANDS_BOTH) {  // the sigma of the band that is not filtered is not read
      clip = opts->bands == DSX_STREAKS_BANDS_FG ? dsx::st::kStFg : dsx::st::kStBg;
      one_sided = *cfg_in;
      if (clip == dsx::st::kStFg) one_sided.sigma_bg = one_sided.sigma_fg;
      else one_sided.sigma_fg = one_sided.sigma_bg;
      cfg = &one_sided;
    }
  }
  if (route != DSX_STREAKS_GENERIC && route != DSX_STREAKS_MARCH) return fail(ctx, DSX_EINVAL, "unknown streaks route");
  if (!cfg) return fail(ctx, DSX_EINVAL, "config is NULL");
  if (height < 1 || width < 1) return fail(ctx, DSX_EINVAL, "plane must be at least 1 x 1");
  if (max_batch < 1) return fail(ctx, DSX_EINVAL, "max_batch must be >= 1");
  if (!(cfg->sigma_fg > 0.f) || !(cfg->sigma_bg > 0.f)) return fail(ctx, DSX_EINVAL, "sigma must be positive");
  if (!(cfg->crossover > 0.f)) return fail(ctx, DSX_EINVAL, "crossover must be positive");
  if (cfg->level < 0) return fail(ctx, DSX_EINVAL, "level must be >= 0");
  if (cfg->otsu == 0 && !(fabsf(cfg->threshold) < 1e30f)) return fail(ctx, DSX_EINVAL, "threshold is not finite");
  if (cfg->wavelet != DSX_WAVELET_DB3 && cfg->wavelet != DSX_WAVELET_BANK)
    return fail(ctx, DSX_EINVAL, "unknown wavelet id");
  if (cfg->wavelet == DSX_WAVELET_BANK && !ctx->wl_set)
    return fail(ctx, DSX_EINVAL, "DSX_WAVELET_BANK needs a filter bank (dsx_set_wavelet)");
  if ((size_t)height * width > ((size_t)1 << 30)) return fail(ctx, DSX_ELIMIT, "plane larger than 2^30 pixels");
  const bool march = route == DSX_STREAKS_MARCH;
  if (march && cfg->wavelet != DSX_WAVELET_DB3)
    return fail(ctx, DSX_EINVAL, "the march route of the streaks plan takes the db3 wavelet only");
  if (march && ((height | width) & 1))
    return fail(ctx, DSX_EINVAL, "the march route of the streaks plan takes planes of even height and width only");
  if (march && max_batch > (1 << 29)) return fail(ctx, DSX_EINVAL, "max_batch too large");
  if (march && cfg->level > std::min(dsx::dwt_max_level(height), dsx::dwt_max_level(width)))
    return fail(ctx, DSX_EINVAL, "the march route of the streaks plan takes levels up to the maximum level only");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  free_plan_buffers(ctx);
  free_streaks(ctx);
  free_lightsheet(ctx);
  ctx->rot = rot;
  ctx->rot_H = height_in;
  ctx->rot_W = width_in;
  dsx::st::StreaksPlan& p = ctx->sp;
  p = dsx::st::StreaksPlan();
  p.H = height; p.W = width; p.B = max_batch;
  p.bands = cfg->sigma_fg == cfg->sigma_bg ? 1 : 2;  // (a one-sided plan: the two are the filtered band's sigma)
  p.clip = clip;
  p.sigma[0] = p.bands == 1 ? cfg->sigma_fg : cfg->sigma_bg;
  p.sigma[1] = cfg->sigma_fg;
  p.crossover = cfg->crossover;
  p.otsu = cfg->otsu ? 1 : 0;
  p.threshold = cfg->threshold;
  if (cfg->wavelet == DSX_WAVELET_DB3) {
    static const double db3[6] = {0.03522629188570953, -0.08544127388202666, -0.13501102001025458,
                                  0.45987750211849154, 0.8068915093110925,   0.33267055295008263};
    p.F = 6;
    for (int t = 0; t < 6; ++t) {
      p.dec.lo[t] = (float)db3[t];
      p.dec.hi[t] = (float)((t & 1 ? 1.0 : -1.0) * db3[5 - t]);  // dec_hi[t] = (-1)^(t+1) dec_lo[F-1-t]
      p.rec.lo[t] = (float)db3[5 - t];
      p.rec.hi[t] = (float)((t & 1 ? -1.0 : 1.0) * db3[t]);       // rec_hi = dec_hi reversed
    }
  } else {
    p.F = ctx->wl_bank_len;
    for (int t = 0; t < p.F; ++t) {
      p.dec.lo[t] = ctx->wl_bank[0][t];
      p.dec.hi[t] = ctx->wl_bank[1][t];
      p.rec.lo[t] = ctx->wl_bank[2][t];
      p.rec.hi[t] = ctx->wl_bank[3][t];
    }
  }
  auto alloc = [&](void** ptr, size_t bytes) -> int {
    hipError_t e = hipMalloc(ptr, std::max<size_t>(bytes, 4));
    if (e != hipSuccess) {
      *ptr = nullptr;
      free_streaks(ctx);
      if (march) free_plan_buffers(ctx);
      return fail(ctx, DSX_ENOMEM, std::string("hipMalloc (streaks plan): ") + hipGetErrorString(e));
    }
    return DSX_OK;
  };
  // the options of the blend: state of the context, and the shading planes on the device
  auto apply_opts = [&]() -> int {
    if (!has_opts) return DSX_OK;
    ctx->st_mode = clip ? clip : p.bands == 1 ? dsx::st::kStSingle : dsx::st::kStBoth;
    ctx->st_R = opts->smoothing > 0.f ? dsx::st::st_smooth_radius((double)opts->smoothing) : 0;
    if (ctx->st_R > 0) dsx::st::st_smooth_taps((double)opts->smoothing, ctx->st_R, ctx->st_taps);
    if (opts->flat) {
      const size_t fb = sizeof(float) * (size_t)height * width;
      const size_t db = rot ? fb : sizeof(float) * (size_t)opts->dark_h * opts->dark_w;
      if (int rc = alloc((void**)&ctx->st_flat, fb)) return rc;
      if (int rc = alloc((void**)&ctx->st_dark, db)) return rc;
      if (rot) {  // the planes are the caller's: dark cropped to the plane, then both turned with the plane
        std::vector<float> rflat, rdark;
        rotate_shading(opts->flat, opts->dark, opts->dark_w, height_in, width_in, rflat, rdark);
        DSX_HIP(hipMemcpy(ctx->st_flat, rflat.data(), fb, hipMemcpyHostToDevice));
        DSX_HIP(hipMemcpy(ctx->st_dark, rdark.data(), db, hipMemcpyHostToDevice));
        ctx->st_dark_w = width;
      } else {
        DSX_HIP(hipMemcpy(ctx->st_flat, opts->flat, fb, hipMemcpyHostToDevice));
        DSX_HIP(hipMemcpy(ctx->st_dark, opts->dark, db, hipMemcpyHostToDevice));
        ctx->st_dark_w = opts->dark_w;
      }
    }
    ctx->st_opts = true;
    return DSX_OK;
  };
  if (march) {
    // band(z, sigma) = log_space_fft_filtering(z, sigma min(H, W) / H, empty mask) - 2: the two filters differ in the
    // normalisation of s only (h sigma / H against h sigma / min(H, W)); cfg 0 = foreground (or the single) band
    const double scale = (double)std::min(height, width) / (double)height;
    for (int c = 0; c < 2; ++c) {
      ctx->cfg[c].level = cfg->level == 0 ? -1 : cfg->level;
      ctx->cfg[c].sigma = (double)(c == 0 ? cfg->sigma_fg : cfg->sigma_bg) * scale;
      ctx->cfg[c].max_threshold = 0.0;  // not read: k_otsu is not launched
    }
    p.Hp = height; p.Wp = width;
    const int P = p.bands * max_batch;
    if (int rc = plan_chain(ctx, height, width, P, false, 0.0, nullptr, nullptr, 0, 0)) return rc;
    p.L = ctx->plan.L;
    // uint16 planes keep uint16 bands when t is integral: Otsu of a uint16 plane always is, a fixed value may not be
    const bool integral = p.otsu || (p.threshold >= 0.f && p.threshold <= 65535.f && p.threshold == floorf(p.threshold));
    ctx->st_vdtype = integral ? DSX_U16 : DSX_F32;
    const size_t px = (size_t)height * width;
    ctx->st_march = true;  // (free_streaks clears it again when an allocation fails)
    if (int rc = alloc(&ctx->st_vin, px * P * sizeof(float))) return rc;  // float32 planes may come with either plan
    if (int rc = alloc((void**)&ctx->st_vout, px * P * sizeof(float))) return rc;
    if (int rc = alloc((void**)&ctx->st_mm, sizeof(unsigned) * 2 * max_batch)) return rc;
    if (int rc = alloc((void**)&ctx->st_hist, sizeof(unsigned) * dsx::st::kStBins * max_batch)) return rc;
    if (int rc = alloc((void**)&ctx->st_t, sizeof(float) * max_batch)) return rc;
    if (int rc = alloc((void**)&ctx->st_info, sizeof(dsx::st::OtsuOut) * max_batch)) return rc;
    ctx->workspace_bytes += 2 * px * P * sizeof(float);
    if (int rc = apply_opts()) return rc;
    ctx->streaks = true;
    ctx->last_n = 0;
    return DSX_OK;
  }
  if (!dsx::st::st_build_plan(p, cfg->level)) return fail(ctx, DSX_ELIMIT, "decomposition level out of range");
  for (int l = 0; l < p.L; ++l)
    if ((size_t)max_batch * p.lv[l].h > (size_t)65535 * dsx::st::kMmT)
      return fail(ctx, DSX_ELIMIT, "max_batch too large for this plane height");
  std::vector<float> mats(std::max<size_t>(p.mat_floats, 1));
  for (int l = 0; l < p.L; ++l)
    for (int b = 0; b < p.bands; ++b)
      dsx::st::st_notch_factors(p.lv[l].w, (double)p.lv[l].h * p.sigma[b] / p.Hp, p.lv[l].rank[b],
                                mats.data() + p.lv[l].mat[b], mats.data() + p.lv[l].mat[b] + (size_t)p.lv[l].w * p.lv[l].rank[b]);
  if (int rc = alloc((void**)&ctx->st_ws, sizeof(float) * p.ws_floats)) return rc;
  if (int rc = alloc((void**)&ctx->st_mat, sizeof(float) * mats.size())) return rc;
  if (int rc = alloc((void**)&ctx->st_mm, sizeof(unsigned) * 2 * max_batch)) return rc;
  if (int rc = alloc((void**)&ctx->st_hist, sizeof(unsigned) * dsx::st::kStBins * max_batch)) return rc;
  if (int rc = alloc((void**)&ctx->st_t, sizeof(float) * max_batch)) return rc;
  if (int rc = alloc((void**)&ctx->st_info, sizeof(dsx::st::OtsuOut) * max_batch)) return rc;
  DSX_HIP(hipMemcpy(ctx->st_mat, mats.data(), sizeof(float) * mats.size(), hipMemcpyHostToDevice));
  if (int rc = apply_opts()) return rc;
  ctx->streaks = true;
  ctx->last_n = 0;
  return DSX_OK;
}

int dsx_plan_lightsheet(dsx_ctx* ctx, int height_in, int width_in, int max_batch, double p, int A, int B, double lambda,
                        const uint32_t* edges, const float* back) {
  using namespace dsx::ls;
  if (!ctx) return DSX_EINVAL;
  if (const char* e = lightsheet_args(height_in, width_in, p, A, B, lambda, edges, back)) return fail(ctx, DSX_EINVAL, e);
  if (max_batch < 1 || max_batch > 65535) return fail(ctx, DSX_EINVAL, "max_batch must be in 1 .. 65535");
  if ((size_t)height_in * width_in > ((size_t)1 << 30)) return fail(ctx, DSX_ELIMIT, "plane larger than 2^30 pixels");
  // dsx_set_rotate: the kernels see np.rot90 of the caller's plane, [width_in, height_in]
  const bool rot = ctx->rot_next;
  const int height = rot ? width_in : height_in, width = rot ? height_in : width_in;
  if ((height + kLsRows - 1) / kLsRows > 65535) return fail(ctx, DSX_ELIMIT, "plane too high for the light-sheet plan");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  free_plan_buffers(ctx);
  free_streaks(ctx);
  free_lightsheet(ctx);
  ctx->rot = rot;
  ctx->rot_H = height_in;
  ctx->rot_W = width_in;
  ctx->ls_H = height; ctx->ls_W = width; ctx->ls_A = A; ctx->ls_B = B;
  ctx->ls_p = p;
  ctx->ls_lambda = (float)lambda;
  ctx->max_batch = max_batch;
  const size_t planes = (size_t)height * width * max_batch;
  void** bufs[5] = {(void**)&ctx->ls_edges, (void**)&ctx->ls_back, (void**)&ctx->ls_q, (void**)&ctx->ls_ls, (void**)&ctx->ls_bg};
  const size_t bytes[5] = {sizeof(uint32_t) * kLsEdges, sizeof(float) * 256, planes, planes, planes};
  for (int k = 0; k < 5; ++k) {
    hipError_t e = hipMalloc(bufs[k], bytes[k]);
    if (e != hipSuccess) {
      *bufs[k] = nullptr;
      free_lightsheet(ctx);
      return fail(ctx, DSX_ENOMEM, std::string("hipMalloc (light-sheet plan): ") + hipGetErrorString(e));
    }
  }
  DSX_HIP(hipMemcpy(ctx->ls_edges, edges, bytes[0], hipMemcpyHostToDevice));
  DSX_HIP(hipMemcpy(ctx->ls_back, back, bytes[1], hipMemcpyHostToDevice));
  ctx->workspace_bytes = 3 * planes;
  ctx->lightsheet = true;
  ctx->last_n = 0;
  return DSX_OK;
}

int dsx_lightsheet_ref(const void* x, int height, int width, double p, int A, int B, double lambda,
                       const uint32_t* edges, const float* back, uint8_t* ls, uint8_t* bg, void* out, int out_dtype) {
  using namespace dsx::ls;
  if (const char* e = lightsheet_args(height, width, p, A, B, lambda, edges, back)) return fail(nullptr, DSX_EINVAL, e);
  if (!x || !out) return fail(nullptr, DSX_EINVAL, "lightsheet: NULL pointer");
  if ((uintptr_t)x & 1) return fail(nullptr, DSX_EINVAL, "lightsheet: uint16 planes must be 2-byte aligned");
  if (out_dtype != DSX_U16 && out_dtype != DSX_F32) return fail(nullptr, DSX_EINVAL, "unknown output type");
  const size_t n = (size_t)height * width;
  std::vector<uint8_t> work(n * 3);
  uint8_t* lsp = ls ? ls : work.data() + n;
  uint8_t* bgp = bg ? bg : work.data() + 2 * n;
  if (out_dtype == DSX_U16)
    lightsheet_host((const uint16_t*)x, height, width, p, A, B, (float)lambda, edges, back, work.data(), lsp, bgp, (uint16_t*)out);
  else
    lightsheet_host((const uint16_t*)x, height, width, p, A, B, (float)lambda, edges, back, work.data(), lsp, bgp, (float*)out);
  return DSX_OK;
}

int dsx_get_lightsheet_planes(dsx_ctx* ctx, int plane, uint8_t* ls, uint8_t* bg) {
  if (!ctx) return DSX_EINVAL;
  if (!ctx->lightsheet) return fail(ctx, DSX_ENOPLAN, "dsx_plan_lightsheet has not been called");
  if (plane < 0 || plane >= ctx->last_n) return fail(ctx, DSX_EINVAL, "plane index out of range");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  const size_t n = (size_t)ctx->ls_H * ctx->ls_W;
  if (ls) DSX_HIP(hipMemcpy(ls, ctx->ls_ls + n * plane, n, hipMemcpyDeviceToHost));
  if (bg) DSX_HIP(hipMemcpy(bg, ctx->ls_bg + n * plane, n, hipMemcpyDeviceToHost));
  return DSX_OK;
}

int dsx_set_rotate(dsx_ctx* ctx, int on) {
  if (!ctx) return DSX_EINVAL;
  ctx->rot_next = on != 0;
  return DSX_OK;  // takes effect at the next dsx_plan / dsx_plan_streaks*
}

namespace {
const char* rot90_args(const void* src, const void* dst, int dtype, int n, int H, int W, int dir) {
  if (n < 0 || H < 1 || W < 1) return "rot90: n must be >= 0 and the plane at least 1 x 1";
  if (dtype != DSX_U16 && dtype != DSX_F32) return "unknown element type";
  if (dir != 1 && dir != -1) return "rot90: dir must be +1 or -1";
  if (n > 0 && (!src || !dst)) return "rot90: NULL pointer";
  if (src == dst && n > 0) return "rot90: the planes cannot be turned in place";
  return nullptr;
}
}  // namespace

int dsx_rot90_device(dsx_ctx* ctx, const void* d_src, void* d_dst, int dtype, int n, int H, int W, int dir) {
  if (!ctx) return DSX_EINVAL;
  if (const char* e = rot90_args(d_src, d_dst, dtype, n, H, W, dir)) return fail(ctx, DSX_EINVAL, e);
  DSX_HIP(hipSetDevice(ctx->device));
  rot_planes(use_main(ctx), d_src, d_dst, dtype, n, H, W, dir);
  DSX_HIP(hipGetLastError());
  return DSX_OK;
}

int dsx_rot90_ref(const void* src, void* dst, int dtype, int n, int H, int W, int dir) {
  if (const char* e = rot90_args(src, dst, dtype, n, H, W, dir)) return fail(nullptr, DSX_EINVAL, e);
  if (dtype == DSX_U16) dsx::rot::rot90_host((const uint16_t*)src, (uint16_t*)dst, n, H, W, dir);
  else dsx::rot::rot90_host((const float*)src, (float*)dst, n, H, W, dir);
  return DSX_OK;
}

int dsx_get_streaks_threshold(dsx_ctx* ctx, int plane, float* threshold) {
  if (!ctx || !threshold) return DSX_EINVAL;
  if (!ctx->streaks) return fail(ctx, DSX_ENOPLAN, "dsx_plan_streaks has not been called");
  if (plane < 0 || plane >= ctx->last_n) return fail(ctx, DSX_EINVAL, "plane index out of range");
  DSX_HIP(hipSetDevice(ctx->device));
  DSX_HIP(hipStreamSynchronize(use_main(ctx)));
  DSX_HIP(hipMemcpy(threshold, ctx->st_t + plane, sizeof(float), hipMemcpyDeviceToHost));
  return DSX_OK;
}

int dsx_streaks_blend_ref(const float* x, const float* f, const float* b, int height, int width, float t,
                          float crossover, const dsx_streaks_opts* opts, void* out, int out_dtype) {
  using namespace dsx::st;
  if (!x || !out) return fail(nullptr, DSX_EINVAL, "streaks blend: NULL pointer");
  if (height < 1 || width < 1) return fail(nullptr, DSX_EINVAL, "plane must be at least 1 x 1");
  if (!(crossover > 0.f)) return fail(nullptr, DSX_EINVAL, "crossover must be positive");
  if (out_dtype != DSX_U16 && out_dtype != DSX_F32) return fail(nullptr, DSX_EINVAL, "unknown output type");
  const int mode = opts ? opts->bands : DSX_STREAKS_BANDS_BOTH;
  const float smoothing = opts ? opts->smoothing : 0.f;
  if (mode != kStBoth && mode != kStFg && mode != kStBg) return fail(nullptr, DSX_EINVAL, "unknown streaks band choice");
  if (!(smoothing >= 0.f && smoothing <= 2.f)) return fail(nullptr, DSX_EINVAL, "smoothing must be 0 or a value in (0, 2]");
  if ((mode != kStBg && !f) || (mode != kStFg && !b)) return fail(nullptr, DSX_EINVAL, "streaks blend: a band plane is NULL");
  const float* flat = opts ? opts->flat : nullptr;
  const float* dark = opts ? opts->dark : nullptr;
  if ((flat == nullptr) != (dark == nullptr)) return fail(nullptr, DSX_EINVAL, "flatfield and darkfield must be given together");
  if (flat && (opts->dark_h < height || opts->dark_w < width))
    return fail(nullptr, DSX_EINVAL, "Please, check the shape of the darkfield.");
  const int dark_w = flat ? opts->dark_w : 0;
  if (out_dtype == DSX_U16)
    st_blend_host<uint16_t>(x, f, b, height, width, t, 1.0f / crossover, mode, (double)smoothing, flat, dark, dark_w, (uint16_t*)out);
  else
    st_blend_host<float>(x, f, b, height, width, t, 1.0f / crossover, mode, (double)smoothing, flat, dark, dark_w, (float*)out);
  return DSX_OK;
}

}  // extern "C"
