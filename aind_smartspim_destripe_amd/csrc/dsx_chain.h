// dsx_chain.h -- the launch chain's decisions and geometry: which kernels a cohort part runs and with what grids,
// blocks and LDS sizes.  Integer arithmetic over dsx::Plan, the switches of a context, the plane count and one CU
// count: pure C++ (no HIP) like dsx_plan.h, so that tests/test_chain_host.py can hold it with g++ and no GPU.
// dsx.hip (run_cohort and its stages) fills the argument structs and launches what this header decides.
#ifndef DSX_CHAIN_H
#define DSX_CHAIN_H

#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#include "dsx_plan.h"

namespace dsx {

// ---- launch-geometry constants shared by the kernels (dsx_kernels.h, dsx_wavelet.h) and the host code ---------------
constexpr int kMarchCols = 256;                 // input columns per wave
constexpr int kMarchOut = (kMarchCols - 4) / 2;  // 126 coefficient columns per wave
constexpr int kFuseOut = (kMarchOut - 4) / 2;    // 61 level-2 columns per wave of the fused kernel
constexpr int kHistWaves = 8;  // waves per block: they share one 32 KB counter array (LDS is what the 4-stream mix runs short of)
constexpr int kRowMaxWaves = 8;  // waves (row pairs) per block; they share one twiddle table
constexpr int kRowMultiMax = 8;  // levels one k_rowfilter_multi / k_rowfilter_pack launch carries
constexpr int kRowPackMax = 4;     // row pairs one wave of k_rowfilter_pack owns, at most
constexpr int kRowPackValues = 18; // complex values a lane holds in a joint pass of k_rowfilter_pack (the CPL = 18 class)
constexpr int kWideThreads = 512;
constexpr int kWideCpl = 36;                              // complex values per lane
constexpr int kWideMaxLen = kWideThreads * kWideCpl;      // 18 432: transform lengths the kernel takes
constexpr int kRfWaves = 8;
constexpr int kRfRows = 2 * kRfWaves - 2;  // coefficient rows p per block
constexpr int kGenTH = 16, kGenTW = 32;    // coefficients per block of k_fwd_gen
constexpr int kGenOH = 32, kGenOW = 64;    // results per block of k_inv_gen
constexpr size_t kLdsLimit = 160 * 1024;   // LDS of a CU: the dynamic-LDS limit the row-filter and level kernels are raised to
constexpr size_t kC32Bytes = 8;            // sizeof(float2): one complex value of a row buffer

#ifdef __HIPCC__
#define DSX_CHAIN_HD __host__ __device__
#else
#define DSX_CHAIN_HD
#endif
// LDS floats of k_fwd_gen for F taps
inline DSX_CHAIN_HD int gen_fwd_cols(int F) { return 2 * kGenTW + F - 2 + 1; }  // + 1: odd pitch
inline DSX_CHAIN_HD int gen_fwd_rows(int F) { return 2 * kGenTH + F - 2; }
inline size_t gen_fwd_lds_bytes(int F) {
  return sizeof(float) * (size_t)(gen_fwd_rows(F) + 2 * kGenTH) * gen_fwd_cols(F);
}
// ... and of k_inv_gen
inline DSX_CHAIN_HD int gen_inv_krows(int F) { return kGenOH / 2 + F / 2 - 1; }
inline DSX_CHAIN_HD int gen_inv_kcols(int F) { return kGenOW / 2 + F / 2 - 1; }
inline size_t gen_inv_lds_bytes(int F) {
  return sizeof(float) * 2 * (size_t)gen_inv_krows(F) * (gen_inv_kcols(F) + 1 + kGenOW + 1);
}

}  // namespace dsx

// Launch-geometry switches of a context, read from the environment ONCE PER CONTEXT by dsx_init (INTEGRATION.md
// section 6).  None of them may change a result: tools/fuzz_parity.py draws them per case (a fresh context each) and
// tests/test_gpu_fuzz.py holds 30 such cases to the parity statement; out-of-range values are clamped here.
struct DsxTuning {
  int row_wpb = 0;            // DSX_ROW_WPB: waves per k_rowfilter block (0 = chosen per transform length)
  int march_waves = 256 * 16; // DSX_MARCH_WAVES: waves a march launch aims at
  bool no_quant = false;      // DSX_NO_QUANT: segment counts without the launch-quantisation score
  int seg_min_rows = 4;       // DSX_SEG_MIN_ROWS: least rows per march segment of the plain level kernels
  bool no_fuse = false;       // DSX_NO_FUSE: one forward launch per level (aa_1 materialised)
  bool no_fuse_inv = false;   // DSX_NO_FUSE_INV: one inverse launch per level
  bool no_pair = false;       // DSX_NO_PAIR: 8-byte pixel / result accesses in the final kernels
  bool no_fuse_rf = false;    // DSX_NO_FUSE_RF: k_rowfilter + k_inv_march instead of k_rowfinal (same bits)
  bool fuse_rf_wide = false;  // DSX_FUSE_RF_WIDE: k_rowfinal for 2000- / 1800-wide planes too (slower there; rowfinal_plan)
  int hist_rows = 0;          // DSX_HIST_ROWS: rows per k_hist block (0 = chosen per cohort size)
  int fwd_wpb = 8, inv_wpb = 8;  // DSX_FWD_WPB / DSX_INV_WPB: waves per block of the fused march kernels (4 or 8)
  bool no_row_multi = false;  // DSX_NO_ROW_MULTI: one row-filter launch per coarse level
  int row_multi_alone = 48;   // DSX_ROW_MULTI_ALONE: largest unsplit cohort that takes the merged coarse row filter
  bool no_row_pack = false;   // DSX_NO_ROW_PACK: k_rowfilter_multi (one row pair per wave) for the merged launch (same bits)
  int row_pack = 0;           // DSX_ROW_PACK: row pairs per wave of k_rowfilter_pack (0 = chosen per level by the cost model)
  int row_pack_wpb = 4;       // DSX_ROW_PACK_WPB: waves per block of k_rowfilter_pack (4 or 8)
  int row_pack_fill = 16;     // DSX_ROW_PACK_FILL: waves per CU (one pair each) from which the merged launch is packed
  int helper = -1;            // DSX_HELPER: -1 = helper stream for unsplit cohorts only, 0 / 1 = never / always
  bool no_pipeline = false;   // DSX_NO_PIPELINE: join the sub-cohort streams at every call
  bool median_lockstep = false;  // DSX_MEDIAN_LOCKSTEP: rf_pair_body counts both rows of a masked pair until both medians are found
                                 // (same bits: tests/test_gpu_median_rows.py; A/B runs)
#ifdef DSX_DIAG
  int skip_hist = 0, skip_row = 0, skip_from = 1000;  // timing-only: WRONG results (DSX_SKIP_HIST / _ROW / _COARSE)
#endif
};

namespace dsx {

inline int env_int(const char* name, int fallback) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : fallback;
}

inline void read_tuning(DsxTuning& t) {
  t.row_wpb = env_int("DSX_ROW_WPB", 0);
  if (t.row_wpb != 0) t.row_wpb = std::max(4, std::min(t.row_wpb, (int)kRowMaxWaves));
  t.march_waves = std::max(64, env_int("DSX_MARCH_WAVES", 256 * 16));
  t.no_quant = env_int("DSX_NO_QUANT", 0) != 0;
  t.seg_min_rows = std::max(2, env_int("DSX_SEG_MIN_ROWS", 4));
  t.no_fuse = env_int("DSX_NO_FUSE", 0) != 0;
  t.no_fuse_inv = env_int("DSX_NO_FUSE_INV", 0) != 0;
  t.no_pair = env_int("DSX_NO_PAIR", 0) != 0;
  t.no_fuse_rf = env_int("DSX_NO_FUSE_RF", 0) != 0;
  t.fuse_rf_wide = env_int("DSX_FUSE_RF_WIDE", 0) != 0;
  t.hist_rows = std::max(0, env_int("DSX_HIST_ROWS", 0));
  t.fwd_wpb = env_int("DSX_FWD_WPB", 8) == 4 ? 4 : 8;
  t.inv_wpb = env_int("DSX_INV_WPB", 8) == 4 ? 4 : 8;
  t.no_row_multi = env_int("DSX_NO_ROW_MULTI", 0) != 0;
  t.row_multi_alone = std::max(0, env_int("DSX_ROW_MULTI_ALONE", 48));
  t.no_row_pack = env_int("DSX_NO_ROW_PACK", 0) != 0;
  t.row_pack = std::max(0, std::min(env_int("DSX_ROW_PACK", 0), (int)kRowPackMax));
  t.row_pack_wpb = env_int("DSX_ROW_PACK_WPB", 4) == 8 ? 8 : 4;
  t.row_pack_fill = std::max(0, env_int("DSX_ROW_PACK_FILL", 16));
  t.helper = getenv("DSX_HELPER") ? (env_int("DSX_HELPER", 0) != 0 ? 1 : 0) : -1;
  t.no_pipeline = env_int("DSX_NO_PIPELINE", 0) != 0;
  t.median_lockstep = env_int("DSX_MEDIAN_LOCKSTEP", 0) != 0;
#ifdef DSX_DIAG
  t.skip_hist = env_int("DSX_SKIP_HIST", 0);
  t.skip_row = env_int("DSX_SKIP_ROW", 0);
  t.skip_from = env_int("DSX_SKIP_COARSE", 1000);
#endif
}

// ---- one row-kernel classifier ---------------------------------------------------------------------------------------
// What a row of a level runs: k_rowfilter_wide, or the k_rowfilter<CPL, GF, NT, HALO, PLAN> instantiation.  gf / nt are
// the slot structure of the row (full 256-value groups, 64-value tail slots), halo says whether the plan embeds the row
// (K > 0), plan the compile-time pass list (a row of kRowPlans): the wide levels of 2048-, 2000- and 1800-wide planes have
// instantiations with all of it as compile-time constants.  gf = nt = halo = -1, plan = 0: the generic body of the class.
struct RowClass {
  bool wide;  // k_rowfilter_wide: rows longer than one wave holds
  int cpl;    // 2, 4, 6, 10, 18, 36
  int gf, nt, halo;
  int plan;   // id of a kRowPlans row, or 0
};

// The compile-time plans, each stated once: the classifier matches a row against them, StaticFft<id> (dsx_kernels.h) runs
// the passes, and the launches of dsx.hip take the template arguments of k_rowfilter / k_rowfinal from here.
struct RowPlan {
  int M, radix[3];    // transform length = radix[0] * radix[1] * radix[2], passes in this order
  int cpl;            // cpl_class(M)
  int gf, nt, halo;   // the row it takes: full 256-value groups, 64-value tail slots, embedded (K > 0) or direct
  bool swz;           // power-of-two passes scatter at power-of-two strides: bank-swizzled addressing (dsx_fft_core.h: dsx_idx_swz)
};
constexpr int kRowPlanCount = 6;
constexpr RowPlan kRowPlans[kRowPlanCount] = {
    {1026, {19, 9, 6}, 18, 4, 1, 0, false},    // 1: level 1 of a 2048-wide plane, direct
    {1071, {17, 9, 7}, 18, 2, 1, 1, false},    // 2: level 2 of a 2048-wide plane: 515 values embedded in 1071
    {2048, {16, 16, 8}, 36, 3, 4, 1, true},    // 3: level 1 of a 2000-wide plane (the production tile): 1002 in 2048
    {1815, {15, 11, 11}, 36, 3, 3, 1, false},  // 4: level 1 of an 1800-wide plane: 902 in 1815
    {1024, {16, 8, 8}, 18, 1, 4, 1, true},     // 5: level 2 of a 2000-wide plane: 503 in 1024
    {960, {15, 8, 8}, 18, 1, 4, 1, false},     // 6: level 2 of an 1800-wide plane: 453 in 960
};
constexpr const RowPlan& row_plan(int id) { return kRowPlans[id - 1]; }

inline RowClass classify_row(int M, int w, int K, int npass, const int* radix) {
  RowClass c = {false, 0, -1, -1, -1, 0};
  const int cpl = (M + 63) / 64;
  if (cpl > 36) { c.wide = true; return c; }
  c.cpl = cpl_class(M);
  const int gf = w >> 8, nt = (w - (gf << 8) + 63) >> 6, halo = K > 0 ? 1 : 0;
  auto set = [&](int plan) { c.gf = gf; c.nt = nt; c.halo = halo; c.plan = plan; };
  for (int id = 1; id <= kRowPlanCount; ++id) {
    const RowPlan& p = row_plan(id);
    if (M == p.M && npass == 3 && radix[0] == p.radix[0] && radix[1] == p.radix[1] && radix[2] == p.radix[2] &&
        c.cpl == p.cpl && gf == p.gf && nt == p.nt && halo == p.halo) {
      set(id);
      return c;
    }
  }
  // two row shapes of the 18-value class have an instantiation with any pass list (plan 0)
  if (c.cpl == 18 && ((gf == 4 && nt == 1 && halo == 0) || (gf == 2 && nt == 1 && halo == 1))) set(0);
  return c;
}
inline RowClass classify_row(const LevelPlan& lp) { return classify_row(lp.M, lp.w, lp.K, lp.npass, lp.radix); }

// Level-1 row filter + final synthesis in one kernel (k_rowfinal): Delta_1 stays in LDS.  Shapes that take it: see the
// kernel's header.  DSX_NO_FUSE_RF=1 keeps the two kernels: A/B runs and the bit-identity test.
// Returns the StaticFft plan id of the instantiation (1, 3, 4) or 0: level 1 classifies as plan 1, or as 3 / 4 with the
// wide switch, and the I/O conditions hold.
inline int rowfinal_plan(const Plan& p, bool in_u16, bool out_u16, bool pair_io, bool wide) {
  const LevelPlan& lp = p.lv[0];
  if (!pair_io || !in_u16 || !out_u16) return 0;
  if ((lp.w & 1) != 0 || (p.Wout + kMarchCols - 1) / kMarchCols > kRfWaves) return 0;
  const int plan = classify_row(lp).plan;
  // wide (DSX_FUSE_RF_WIDE=1; OFF by default): the embedded plans of 2000- and 1800-wide planes.  Their
  // FFT buffers are 16 KB per wave: one 8-wave block per CU, the two phases of a block cannot hide behind another
  // block's, and the fused kernel LOSES 10-12 % against k_rowfilter + k_inv_march there (1600 x 2000: 53.8 k against
  // 59.8 k planes/s, 1800^2: 54.8 k against 62.8 k; profiles/r3_fused_rowfinal_ab.txt).  Bit-identical all the same
  // (tests/test_gpu_parity.py::test_fused_rowfinal_is_bit_identical_to_the_unfused_chain runs them with the switch on).
  if (plan == 1 || (wide && (plan == 3 || plan == 4))) return plan;
  return 0;
}

// ---- a cohort and its parts --------------------------------------------------------------------------------------------
// Parts (sub-cohort streams) a cohort of nb planes runs as; one_chain: profiling, staged debug runs and stack mode (one
// control block, one chain) do not split
inline int cohort_parts(int n_streams, int nb, bool one_chain) {
  int parts = one_chain ? 1 : n_streams;
  while (parts > 1 && nb / parts < 16) --parts;  // keep every part big enough to fill the chip
  return parts;
}

// 1 = a part may use its helper stream.  Measured at 2048^2: a cohort that runs as ONE
// part gains 6 % (52.5 k against 49.5 k planes/s), a cohort split over 4 streams LOSES 2-8 % (the other parts
// already fill the chip, the extra streams only add contention), so only unsplit cohorts use it; DSX_HELPER=0 / 1
// forces it off / on.  Never for profiled or staged runs.
inline bool part_uses_helper(const DsxTuning& t, bool alone, bool profiled_or_staged) {
  const bool use = t.helper >= 0 ? t.helper != 0 : alone;
  return use && !profiled_or_staged;
}

// ---- the chain's shape -----------------------------------------------------------------------------------------------
struct ChainCall {     // what one cohort part brings
  bool in_u16, out_u16;
  int nb;              // planes of the part
  bool aligned16;      // input and result are 16-byte aligned
  bool bank;           // a filter bank other than db3 (dsx_set_wavelet)
  int stop_after;      // staged debug runs (dsx_set_stop_after)
  bool st_march;       // march route of the dual-band filter: thr / cfg come from k_st_chainfill
  bool has_helper;     // the part may use its helper stream
  bool alone;          // the cohort runs as ONE part
};

struct ChainShape {
  bool generic;    // any wavelet but db3: tap-count-generic level kernels, one launch per level, nothing fused
  bool fuse12;     // levels 1 + 2 in one forward kernel (aa_1 never leaves the chip)
  bool fuse21;     // level-2 synthesis inside the final kernel (c_1 never leaves the chip)
  bool pair_io;    // 16-byte pixel / result accesses by lane pairs (inv_march_body<.., PAIR>)
  int rf_plan;     // != 0: level-1 row filter inside the final kernel (k_rowfinal), its StaticFft plan id
  bool split;      // the wide levels' histograms run on the helper stream beside the coarse forward levels
  bool split_inv;  // ... and their row filters beside the coarse row filters and inverse levels
  bool thresholds; // k_hist / k_otsu run (not for the march route of the dual-band filter)
  bool multi;      // coarse levels on the part's own stream may share ONE row-filter launch (k_rowfilter_multi)
};

inline ChainShape chain_shape(const Plan& p, const DsxTuning& t, const ChainCall& c) {
  ChainShape s;
  const int L = p.L;
  s.generic = c.bank && L > 0;
  // levels 1 + 2 in one kernel when the plane allows it
  s.fuse12 = !s.generic && !t.no_fuse && L >= 2 && (p.W % 4) == 0 && (p.lv[0].ldin % 4) == 0 && p.lv[0].h >= 16 &&
             p.lv[0].w >= 16;
  s.fuse21 = s.fuse12 && !t.no_fuse_inv;
  // uint16 planes whose rows and bases allow 16-byte pixel / result accesses by lane pairs
  s.pair_io = !t.no_pair && c.in_u16 && (p.W % 8) == 0 && (p.H % 2) == 0 && p.Wout == p.W && c.aligned16 &&
              ((size_t)p.H * p.W * 2) % 16 == 0;
  // level-1 row filter inside the final kernel (k_rowfinal): not for the staged debug runs, which read Delta_1 back
  s.rf_plan = (s.fuse21 && !t.no_fuse_rf && c.stop_after == 0) ? rowfinal_plan(p, c.in_u16, c.out_u16, s.pair_io, t.fuse_rf_wide) : 0;
  // The wide levels (1, 2) hold 94 % of the coefficients; the coarse levels are chains of small launches that
  // leave most of the chip idle.  With the fused forward kernel the wide levels' data is complete early, so
  // their histograms (and their row filters) run on the part's helper stream BESIDE the coarse
  // levels' launches instead of after them.
  s.split = c.has_helper && s.fuse12 && L >= 3;
  // row filters: levels 1, 2 on the helper stream (1.5 ms of the 5.3 ms chain per 256 planes), the coarse levels'
  // row filters AND the coarse inverse levels on the part's own stream beside them; joined before the final kernel
  s.split_inv = s.split && s.fuse21;  // the fused final kernel consumes Delta_1, Delta_2 and c_2 only
  s.thresholds = !c.st_march;  // no mask: thr / cfg come from k_st_chainfill
  // coarse levels (M <= 384) that run on the part's own stream: one launch for all of them (DSX_NO_ROW_MULTI=1: one each)
  // (only for cohorts split over the streams, where the launch gaps of six small kernels cost more than the
  //  specialised CPL = 2 / 4 instantiations save: +2.4 % there, -5 % for a cohort that runs alone -- its coarse chain
  //  is the critical path beside the level-2 row filter on the helper stream; profiles/r3_merged_small_launches_ab.txt)
  // ... and small cohorts that run alone are launch-bound again: one plane 418 -> 358 us per call, 32 planes + 7 %,
  // 64 planes even, 128 planes - 2.7 % (profiles/r3_merged_small_launches_ab.txt); DSX_ROW_MULTI_ALONE = the limit
  s.multi = !t.no_row_multi && (!c.alone || c.nb <= t.row_multi_alone);
  return s;
}

// a level whose row filter joins the merged coarse launch (nlev: levels it holds already)
inline bool row_multi_takes(const ChainShape& s, bool own_stream, int M, int nlev) {
  return s.multi && own_stream && M <= 6 * 64 && nlev < kRowMultiMax;
}

// ---- k_zero3 -------------------------------------------------------------------------------------------------------------
// The control block of a part (stats | minmax | hist) in 16-byte words: stats 256 B per plane; minmax 8 Lc B per plane
// (parts start at even planes -> 16-byte aligned except for odd Lc * po: grid_x = 0, three memsets instead of the
// kernel); hist 1 KiB per plane and level
constexpr size_t kPlaneStatsBytes = 256;  // sizeof(PlaneStats)
struct ZeroLaunch {
  int n0, n1, n2;  // 16-byte words of stats, minmax, hist
  int grid_x;      // blocks of 256 lanes; 0: the minmax slice is not 16-byte aligned
};
inline ZeroLaunch zero_launch(int nb, int Lc, size_t minmax_addr) {
  const size_t mm_bytes = sizeof(unsigned) * 2 * Lc * (size_t)nb;
  ZeroLaunch z = {(int)(kPlaneStatsBytes * nb / 16), (int)(mm_bytes / 16), (int)(sizeof(unsigned) * 256 * Lc * (size_t)nb / 16), 0};
  if ((mm_bytes % 16) == 0 && (minmax_addr % 16) == 0) z.grid_x = std::min((z.n0 + z.n1 + z.n2 + 255) / 256, 1024);
  return z;
}

// ---- march kernels -----------------------------------------------------------------------------------------------------
struct MarchSeg {
  int nseg, rows_per_seg;
};

// Row segmentation of the marching kernels: enough waves to fill the chip for small cohorts,
// one segment per strip for large ones (each extra segment re-reads a 4-row halo).
// wpb > 0 (the fused level-1 kernels, wpb waves per block, 16 waves per CU): the segment count is also chosen against
// the QUANTISATION of the launch -- blocks run in rounds of (CUs x 16 / wpb); 576 equal blocks on 512 slots take two
// rounds, 512 take one.  Among the counts around the target the one with the smallest rounds x (rows per segment +
// halo_rows) wins (halo_rows: the rows a segment recomputes, in the units of `rows`).
// cus: compute units of the device (dsx_init asks once per context; 256 when the device does not say).
inline MarchSeg march_segments(const DsxTuning& t, int cus, int nb, int nstrips, int rows, int wpb = 0, int halo_rows = 0,
                               bool coarse = false) {
  int want = (t.march_waves + nb * nstrips - 1) / (nb * nstrips);
  // Rows per segment, at least: 24 until late in round 3.  The coarse levels (260 rows and fewer) then ran as a few
  // hundred waves marching 24+ rows each -- launches that are short on parallelism, not on work: levels 3 ... 8 hold 6 % of
  // the coefficients and cost 19 % of the run (timing-only DSX_SKIP_COARSE, profiles/r3_coarse_levels.txt).  4 rows per
  // segment (2 more of halo) gives them 3-6 x the waves and a march a sixth as long: +0.8 % on the whole run.  Only the
  // plain level kernels take it (coarse = true); the fused level-1 + 2 kernels keep 24: at the cohort sizes that matter
  // their segment count is set by the wave target, not by this floor.  (The first attempt gave them 4 rows too and failed
  // the GPU suite -- through last segments of one or two level-2 rows, the bug fwd_march_body's i_first now fixes.)
  const int seg_min_rows = coarse ? t.seg_min_rows : 24;
  const int max_seg = std::max(1, rows / seg_min_rows);
  want = std::max(1, std::min(want, max_seg));
  if (wpb > 0 && !t.no_quant) {
    const long long slots = (long long)cus * (16 / wpb);
    double best = 1e300;
    int best_n = want;
    for (int n = std::max(1, want / 2); n <= std::min(max_seg, 2 * want + 1); ++n) {
      const int rps = (rows + n - 1) / n;
      const int ns = (rows + rps - 1) / rps;
      const long long blocks = (long long)nb * ((nstrips * ns + wpb - 1) / wpb);
      const long long rounds = (blocks + slots - 1) / slots;
      // a launch that leaves most of the chip empty is no bargain either: count at least half a round
      const double fill = std::max(0.5, (double)blocks / (double)slots);
      const double cost = std::max((double)rounds, fill) * (double)(rps + halo_rows);
      if (cost < best * 0.999) { best = cost; best_n = n; }
    }
    want = best_n;
  }
  int rps = (rows + want - 1) / want;
  rps = std::max(1, std::min(rps, 4096));  // uint32 partial sums of k_fwd1_march
  return {(rows + rps - 1) / rps, rps};
}

struct MarchLaunch {
  int nstrips, nseg, rows_per_seg;
  int wpb;     // waves per block: 4, or 8 for the fused kernels (DSX_FWD_WPB / DSX_INV_WPB = 4 restores 4)
  int grid_x;  // blocks per plane
};

inline MarchLaunch march_launch(int nstrips, MarchSeg g, int wpb) {
  return {nstrips, g.nseg, g.rows_per_seg, wpb, (nstrips * g.nseg + wpb - 1) / wpb};
}

// forward level l (index; not the level-2 half of the fused kernel, which level 0 carries)
inline MarchLaunch fwd_launch(const Plan& p, const ChainShape& s, const DsxTuning& t, int cus, int nb, bool alone, int l) {
  if (s.fuse12 && l == 0) {
    const LevelPlan& l2 = p.lv[1];
    const int nstrips = (l2.w + kFuseOut - 1) / kFuseOut;
    // (a cohort split over the streams shares the chip with the other parts' kernels: rounds mean nothing there --
    //  measured 65.6 k with against 66.2 k planes/s without; alone: forward kernel 1.39 -> 1.14 ms per 256 planes)
    // 8 waves per block for the fused kernels: a block covers 8 consecutive strips of one row segment (4 KB of
    // contiguous pixels per row at 2048 columns), and at most 8 march waves sit on a CU next to the other
    // streams' row-filter blocks: +4 % in the 4-stream run (DSX_FWD_WPB / DSX_INV_WPB = 4 restores 4)
    return march_launch(nstrips, march_segments(t, cus, nb, nstrips, l2.h, alone ? 8 : 0, 2), t.fwd_wpb);
  }
  const LevelPlan& lp = p.lv[l];
  const int nstrips = (lp.w + kMarchOut - 1) / kMarchOut;
  return march_launch(nstrips, march_segments(t, cus, nb, nstrips, lp.h, 0, 0, /*coarse=*/l >= 2), 4);
}

// inverse level l (l <= 0: the final kernel); hout x wout is what the launch writes
inline MarchLaunch inv_launch(const ChainShape& s, const DsxTuning& t, int cus, int nb, int l, int hout, int wout) {
  const int nstrips = (wout + kMarchCols - 1) / kMarchCols;
  MarchSeg g = march_segments(t, cus, nb, nstrips, (hout + 1) / 2, 0, 0, /*coarse=*/l >= 2);
  const bool fused = s.fuse21 && l <= 0;
  if (fused && (g.rows_per_seg & 1)) {  // segments start at even level-1 rows
    g.rows_per_seg += 1;
    g.nseg = ((hout + 1) / 2 + g.rows_per_seg - 1) / g.rows_per_seg;
  }
  return march_launch(nstrips, g, fused ? t.inv_wpb : 4);
}

// ---- k_hist ------------------------------------------------------------------------------------------------------------
// rows per block: each block zeroes and folds 32 KB of counters, so big cohorts take tall blocks (128 rows: + 1-2 %
// in the 4-stream run against 32), small ones keep enough blocks to spread over the chip (~512 per launch)
inline int hist_rows_per_block(const DsxTuning& t, int h, int w, int nb) {
  const int auto_rows = std::max(32, std::min(128, (int)((long long)h * nb / 512)));
  // k_hist counts in 16-bit per-lane counters shared by the waves of a block: a lane sees 4 values per 16-byte load
  // and (w >> 8) + 1 loads per row at most, and in the worst case they all fall into ONE bin (bin 0 of a plane with
  // one outlier) -- the rows of a block are capped so that even then no counter carries into its neighbour
  // (w = 18 432, the widest level k_rowfilter_wide admits: 227 rows)
  const int rows_cap = std::min(256, 65535 / (4 * (w >> 8) + 4));
  return std::max(1, std::min(t.hist_rows > 0 ? t.hist_rows : auto_rows, rows_cap));
}

// ---- row filters -------------------------------------------------------------------------------------------------------
// Waves (row pairs) per block: they share one twiddle table in LDS; pick the count that puts the
// most waves on a CU (160 KiB LDS, at most 16 waves at 4 waves per SIMD).
inline int rowfilter_waves_per_block(int M) {
  int best_w = 4, best_total = 0;
  for (int w = 4; w <= kRowMaxWaves; ++w) {
    const size_t bytes = (size_t)M * (w + 1) * kC32Bytes;
    const int blocks = (int)std::min<size_t>(kLdsLimit / bytes, 8);
    const int total = std::min(blocks * w, 16);
    if (total > best_total) { best_total = total; best_w = w; }
  }
  return best_w;
}

struct RowLaunch {
  int wpb;      // waves (row pairs) per block
  size_t lds;   // twiddle table + one row buffer per wave
  int grid_x;   // blocks per plane
};

// k_rowfilter<CPL, ...> over npairs row pairs of length-M transforms
inline RowLaunch rowfilter_launch(const DsxTuning& t, int cpl, int M, int npairs) {
  int force_wpb = t.row_wpb;
  if (force_wpb && (size_t)M * (force_wpb + 1) * kC32Bytes > kLdsLimit) force_wpb = 0;  // would not fit the LDS
  // M >= 1024 (level 2 of the hot shapes, 77 KB per 8-wave block): 4-wave blocks of 43 KB.  Alone the kernel does not
  // care; beside the 74 KB blocks of k_rowfinal and the small coarse-level blocks three of them still find room on a CU
  // where two of the big ones do not (+0.6 % 4-stream, +1.3 % single-stream, gpurun_out/wpb_sweep.txt)
  const int wpb = force_wpb ? force_wpb : ((cpl > 18 || M >= 1024) ? 4 : rowfilter_waves_per_block(M));
  return {wpb, (size_t)M * (wpb + 1) * kC32Bytes, (npairs + wpb - 1) / wpb};
}

// k_rowfinal: kRfWaves row pairs per block, of which the last is the first of the next block
inline RowLaunch rowfinal_launch(int M, int hout) {
  const int np = (hout + 1) / 2;
  return {kRfWaves, (size_t)M * (kRfWaves + 1) * kC32Bytes, (np + kRfRows - 1) / kRfRows};
}

// Levels whose row filters all fit the CPL = 6 class, in ONE launch (k_rowfilter_multi): blk_end[i] = blocks of levels
// 0 .. i, the last one is the grid
inline RowLaunch row_multi_launch(int nlev, const int* npairs, const int* M, int* blk_end) {
  const int wpb = kRowMaxWaves;
  int blocks = 0, max_m = 1;
  for (int i = 0; i < nlev; ++i) {
    blocks += (npairs[i] + wpb - 1) / wpb;
    blk_end[i] = blocks;
    max_m = std::max(max_m, M[i]);
  }
  return {wpb, (size_t)max_m * (wpb + 1) * kC32Bytes, blocks};
}

// ---- the merged coarse launch with SEVERAL row pairs per wave (k_rowfilter_pack) -----------------------------------------
// One wave per row pair leaves most lanes of a short row's passes idle: a pass of radix R over M values has M / R
// butterflies, one per lane (M = 260: 20, 52 and 65 of 64 lanes; M = 36: 6 and 6).  A wave of the packed kernel owns P
// consecutive pairs and runs every pass jointly over the P row buffers: virtual butterfly v = lane + 64 i < P M / R.

// v -> (pair, butterfly) without a division: off = pair * stride, b = v - pair * n; for 0 <= v < kRowPackMax * n
inline DSX_CHAIN_HD void row_pack_split(int v, int n, int stride, int& off, int& b) {
  off = 0;
  b = v;
  for (int j = 1; j < kRowPackMax; ++j) {
    if (b >= n) {
      b -= n;
      off += stride;
    }
  }
}

// a pass list the joint passes take: register butterflies only (a generic pass runs pair by pair)
inline bool row_pack_reg_passes(int npass, const int* radix) {
  for (int i = 0; i < npass; ++i) {
    bool reg = false;
    for (int q : kRegRadix) reg = reg || (q == radix[i]);
    if (!reg) return false;
  }
  return true;
}

// modelled cost of the passes of one transform per row pair, P pairs per wave (pass_cost of dsx_plan.h with the rounds
// counted over the P buffers together)
inline double row_pack_cost(int M, int npass, const int* radix, int P) {
  double c = 0;
  for (int i = 0; i < npass; ++i) c += 60.0 + round_cost(radix[i]) * (double)((P * (M / radix[i]) + 63) / 64);
  return c / P;
}

// registers: a lane never holds more than kRowPackValues complex values in a pass; LDS: the twiddle table and P row
// buffers per wave, with 16 waves (16 / wpb blocks) on a CU
inline bool row_pack_fits(int M, int npass, const int* radix, int P, int wpb) {
  for (int i = 0; i < npass; ++i) {
    const int R = radix[i];
    if (P * (M / R) > 64 * ((kRowPackValues + R - 1) / R)) return false;
  }
  return (size_t)(16 / wpb) * (size_t)(1 + wpb * P) * M * kC32Bytes <= kLdsLimit;
}

// Row pairs per wave for a level: the P <= kRowPackMax of least modelled cost within both bounds (the smaller one on a
// tie); DSX_ROW_PACK = n: the largest P <= n within the bounds.  Measured at M = 260, where the model separates
// P = 3 from P = 4 by 6 % only: profiles/row_pack_bench.txt.
inline int row_pack_factor(const DsxTuning& t, int M, int npass, const int* radix) {
  if (!row_pack_reg_passes(npass, radix)) return 1;
  int best = 1;
  double best_cost = row_pack_cost(M, npass, radix, 1);
  for (int P = 2; P <= kRowPackMax; ++P) {
    if (!row_pack_fits(M, npass, radix, P, t.row_pack_wpb)) break;
    if (t.row_pack > 0) {
      if (P <= t.row_pack) best = P;
      continue;
    }
    const double c = row_pack_cost(M, npass, radix, P);
    if (c < best_cost) { best_cost = c; best = P; }
  }
  return t.row_pack == 1 ? 1 : best;
}

// The merged launch goes to k_rowfilter_pack (DSX_NO_ROW_PACK=1: k_rowfilter_multi); a single level runs its own kernel.
// waves: what the launch has with one pair per wave (planes x row pairs of its levels).  Packing trades parallelism for
// lane use, and a launch that does not fill the chip once (16 waves on each of the cus compute units) has idle SIMDs, not
// idle lanes, to give away: its waves would only run 3-4 x as long.  Measured on 2048^2 planes, latency per call: 1 plane
// 250 -> 264 us, 8 planes 313 -> 326 us packed, 16 planes (4224 waves on 256 CUs) even (profiles/row_pack_bench.txt).
// Those launches keep one pair per wave; DSX_ROW_PACK_FILL = 0 packs whatever the size.
inline bool row_pack_runs(const DsxTuning& t, int nlev, long long waves, int cus) {
  return !t.no_row_pack && nlev >= 2 && waves >= (long long)t.row_pack_fill * cus;
}

// k_rowfilter_pack: wpb waves per block, pack[i] row pairs per wave of level i; blk_end as in row_multi_launch
inline RowLaunch row_pack_launch(const DsxTuning& t, int nlev, const int* npairs, const int* M, const int* pack, int* blk_end) {
  const int wpb = t.row_pack_wpb;
  int blocks = 0;
  size_t lds = kC32Bytes;
  for (int i = 0; i < nlev; ++i) {
    const int per_block = wpb * pack[i];
    blocks += (npairs[i] + per_block - 1) / per_block;
    blk_end[i] = blocks;
    lds = std::max(lds, (size_t)(1 + wpb * pack[i]) * M[i] * kC32Bytes);
  }
  return {wpb, lds, blocks};
}

}  // namespace dsx
#endif  // DSX_CHAIN_H
