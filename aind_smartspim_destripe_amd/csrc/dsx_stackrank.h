// dsx_stackrank.h -- per-pixel order statistics of a stack of uint16 planes (gfx950), and its host build.
//
// The reference makes its retrospective flat fields with flatfield_estimation.py: sample tiles are destriped and BaSiC
// fits a flat / dark / baseline to the stack.  BaSiC is not restated here; the estimator of this project
// (aind_smartspim_destripe_amd/flatfield_estimation.py) is a per-pixel quantile of the destriped sample planes, smoothed
// on the host.  The samples lie in device memory as uint16 [n, P] behind the filter, so what the device has to do is one
// order statistic per pixel across the stack, with the stack read from HBM once.
//
// Contract (both builds): n planes of P elements, a validity window lo <= hi, n_q quantiles q in per-mille.  Per pixel
// p, V = the multiset of x[j, p] with lo <= x <= hi, m = |V|; valid[p] = m; out[q, p] = the k-th smallest element of V
// (0-based), k = (q * (m - 1)) / 1000 in INTEGER arithmetic, and 0 where m == 0.  1 <= n <= 512, 1 <= n_q <= 4,
// 1 <= P < 2^31, 0 <= lo <= hi <= 65535, 0 <= q <= 1000.
//
//   k_stack_rank_u16 : one block of 256 threads owns a tile of TP consecutive pixels across all n planes, held in LDS as
//       [n][TP] uint16 (TP * n * 2 <= 64 KiB: TP = 256 for n <= 128, 128 for n <= 256, 64 for n <= 512; with the 4 KiB of
//       partial counts two blocks fit a CU's 160 KiB).  TP * S = 256: thread t is plane slice s = t / TP of pixel
//       t % TP, and because slice s holds the planes s, s + S, ... its values are the tile elements t, t + 256,
//       t + 512, ... -- a fixed stride, consecutive lanes on consecutive halfwords, no bank conflict.
//
//       Load: every plane's segment of the tile is read once, coalesced: 16-byte loads (8 pixels per lane, four in
//       flight) where P % 8 == 0 and the base is 16-byte aligned -- every segment then starts on a 16-byte boundary --
//       and 2-byte loads elsewhere (the stack is only 2-byte aligned and P may be odd).  Values are stored as
//       y = (x - lo) mod 2^16: the valid ones are exactly those with y <= hi - lo, so the select phase needs ONE
//       unsigned compare per value, y < limit, for "valid and below the candidate".
//
//       Select: m = #{y < hi - lo + 1}; then a 16-step bisection over the value domain from the top bit down, all n_q
//       quantiles in the same sweep over the slice (one LDS read serves them all): cand = ans | bit,
//       c = #{y < min(cand, hi - lo + 1)}, ans = cand if c <= k.  The largest v with #{valid y < v} <= k is the k-th
//       smallest valid value.  The S partial counts of a pixel meet in a small LDS array, double-buffered so that a
//       step costs one barrier; with S == 1 there is none.  All compares are unsigned.  Results leave with plain
//       2-byte vector stores; no atomics, no scratch.
//
//   stack_rank_host  : the same contract on the host, plain C++ (sort of the valid values of a pixel).
#ifndef DSX_STACKRANK_H
#define DSX_STACKRANK_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dsx {
namespace sr {

constexpr int kSrThreads = 256;          // threads of a block: TP pixels x S plane slices
constexpr int kSrMaxPlanes = 512;        // n
constexpr int kSrMaxQ = 4;               // quantiles of one call
constexpr size_t kSrTileLimit = 65536;   // bytes of the [n][TP] tile
constexpr size_t kSrPartBytes = 2 * kSrMaxQ * kSrThreads * sizeof(uint16_t);  // partial counts, two buffers
constexpr size_t kSrMaxElems = ((size_t)1 << 31) - 1;                         // P

// The argument rules both builds share; nullptr when the call may run.
inline const char* check_args(const void* planes, int n, size_t plane_elems, int lo, int hi, const int* q_milli, int n_q,
                              const void* out) {
  if (n < 1 || n > kSrMaxPlanes) return "stack_rank: 1 <= n <= 512 planes";
  if (n_q < 1 || n_q > kSrMaxQ) return "stack_rank: 1 <= n_q <= 4 quantiles";
  if (plane_elems < 1 || plane_elems > kSrMaxElems) return "stack_rank: 1 <= plane_elems < 2^31";
  if (lo < 0 || hi > 65535 || lo > hi) return "stack_rank: 0 <= lo <= hi <= 65535";
  if (!planes || !q_milli || !out) return "stack_rank: NULL pointer";
  if ((uintptr_t)planes & 1) return "stack_rank: uint16 planes must be 2-byte aligned";
  for (int i = 0; i < n_q; ++i)
    if (q_milli[i] < 0 || q_milli[i] > 1000) return "stack_rank: a quantile is per-mille, 0 <= q <= 1000";
  return nullptr;
}

// 0-based rank of quantile q (per-mille) among m >= 1 valid values: the integer rule of the contract.
inline unsigned rank_of(unsigned q_milli, unsigned m) { return q_milli * (m - 1u) / 1000u; }

// What a launch over n planes of P elements looks like (n and P inside the limits).
struct Geometry {
  int tp;             // pixels of a tile
  int slices;         // S: threads per pixel
  size_t tile_bytes;  // tp * n * 2
  size_t lds_bytes;   // tile + partial counts: the dynamic LDS of the launch
  size_t grid;        // blocks: tiles that cover P, the last one ragged
};
inline Geometry geometry(int n, size_t plane_elems) {
  Geometry g;
  g.tp = n <= 128 ? 256 : n <= 256 ? 128 : 64;
  g.slices = kSrThreads / g.tp;
  g.tile_bytes = (size_t)g.tp * (size_t)n * sizeof(uint16_t);
  g.lds_bytes = g.tile_bytes + kSrPartBytes;
  g.grid = (plane_elems + (size_t)g.tp - 1) / (size_t)g.tp;
  return g;
}

// Arguments as check_args passed them.  Pixels are taken in runs of kRun so that a plane is read in short rows.
inline void stack_rank_host(const uint16_t* planes, int n, size_t P, int lo, int hi, const int* q_milli, int n_q,
                            uint16_t* out, uint16_t* valid) {
  constexpr size_t kRun = 64;
  std::vector<uint16_t> col(kRun * (size_t)n);
  std::vector<unsigned> cnt(kRun);
  for (size_t p0 = 0; p0 < P; p0 += kRun) {
    const size_t run = std::min(kRun, P - p0);
    std::fill(cnt.begin(), cnt.begin() + run, 0u);
    for (int j = 0; j < n; ++j) {
      const uint16_t* row = planes + (size_t)j * P + p0;
      for (size_t i = 0; i < run; ++i) {
        const int x = row[i];
        if (x >= lo && x <= hi) col[i * (size_t)n + cnt[i]++] = (uint16_t)x;
      }
    }
    for (size_t i = 0; i < run; ++i) {
      uint16_t* v = col.data() + i * (size_t)n;
      const unsigned m = cnt[i];
      std::sort(v, v + m);
      for (int q = 0; q < n_q; ++q) out[(size_t)q * P + p0 + i] = m ? v[rank_of((unsigned)q_milli[q], m)] : (uint16_t)0;
      if (valid) valid[p0 + i] = (uint16_t)m;
    }
  }
}

}  // namespace sr
}  // namespace dsx

#if defined(__HIP__)
#include <hip/hip_runtime.h>

namespace dsx {
namespace sr {

typedef unsigned int sr_u32x4 __attribute__((ext_vector_type(4)));

struct Quantiles {
  int q[kSrMaxQ];
};

// both halfwords of w minus lo, each mod 2^16
__device__ __forceinline__ unsigned sr_sub2(unsigned w, unsigned lo) {
  return ((w - lo) & 0xffffu) | ((w & 0xffff0000u) - (lo << 16));
}

// c[k] = number of the thread's values (tile elements t, t + 256, ... below `elems`) that are < lim[k]
template <int NQ>
__device__ __forceinline__ void sr_count(const uint16_t* mine, int steps, const unsigned (&lim)[NQ], unsigned (&c)[NQ]) {
#pragma unroll
  for (int k = 0; k < NQ; ++k) c[k] = 0u;
#pragma unroll 8
  for (int i = 0; i < steps; ++i) {
    const unsigned y = mine[(size_t)i * kSrThreads];
#pragma unroll
    for (int k = 0; k < NQ; ++k) c[k] += y < lim[k] ? 1u : 0u;
  }
}

// The counts of the S slices of a pixel added up; every thread of the pixel gets the total.  part: [2][NQ][256].
template <int NQ>
__device__ __forceinline__ void sr_combine(uint16_t* part, int& parity, int t, int px, int tp, int slices, unsigned (&c)[NQ]) {
  if (slices == 1) return;  // (the same for the whole block)
  uint16_t* buf = part + parity * (kSrMaxQ * kSrThreads);
#pragma unroll
  for (int k = 0; k < NQ; ++k) buf[k * kSrThreads + t] = (uint16_t)c[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    unsigned sum = 0u;
    for (int s = 0; s < slices; ++s) sum += buf[k * kSrThreads + s * tp + px];
    c[k] = sum;
  }
  parity ^= 1;  // the next step writes the other buffer: one barrier per step is enough
}

// grid: geometry(n, P).grid blocks of kSrThreads threads; dynamic LDS: geometry(n, P).lds_bytes.  tp = 1 << tp_log2.
// vec: P % 8 == 0 and planes is 16-byte aligned.  out: [NQ][P]; valid: [P] or nullptr.  range = hi - lo.
template <int NQ>
__global__ __launch_bounds__(kSrThreads) void k_stack_rank_u16(const uint16_t* __restrict__ planes, int n, size_t P,
                                                               unsigned lo, unsigned range, Quantiles qs,
                                                               uint16_t* __restrict__ out, uint16_t* __restrict__ valid,
                                                               int tp_log2, int vec) {
  extern __shared__ __attribute__((aligned(16))) uint16_t sr_lds[];
  const int tp = 1 << tp_log2, slices = kSrThreads >> tp_log2;
  uint16_t* tile = sr_lds;                                // [n][tp]
  uint16_t* part = sr_lds + (size_t)n * (size_t)tp;       // [2][kSrMaxQ][kSrThreads]
  const int t = threadIdx.x, px = t & (tp - 1);
  const size_t p0 = (size_t)blockIdx.x * (size_t)tp;
  const int np = (int)(P - p0 < (size_t)tp ? P - p0 : (size_t)tp);  // pixels of this tile
  const int elems = n * tp;

  if (vec) {  // np % 8 == 0 here
    const int vlog = tp_log2 - 3, v = t & ((1 << vlog) - 1), rstep = kSrThreads >> vlog;
    const bool col_ok = v * 8 < np;
    for (int j0 = t >> vlog; j0 < n; j0 += 4 * rstep) {
      sr_u32x4 w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * rstep;
        w[u] = (col_ok && j < n) ? *reinterpret_cast<const sr_u32x4*>(planes + (size_t)j * P + p0 + (size_t)v * 8)
                                 : sr_u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * rstep;
        if (col_ok && j < n) {
          const sr_u32x4 y = {sr_sub2(w[u].x, lo), sr_sub2(w[u].y, lo), sr_sub2(w[u].z, lo), sr_sub2(w[u].w, lo)};
          *reinterpret_cast<sr_u32x4*>(tile + j * tp + v * 8) = y;
        }
      }
    }
  } else {  // tile element f = t, t + 256, ...: plane f / tp, pixel px
#pragma unroll 8
    for (int f = t; f < elems; f += kSrThreads) {
      if (px < np) tile[f] = (uint16_t)((unsigned)planes[(size_t)(f >> tp_log2) * P + p0 + (size_t)px] - lo);
    }
  }
  __syncthreads();

  const uint16_t* mine = tile + t;
  const int steps = (elems - t + kSrThreads - 1) / kSrThreads;  // >= 1: elems is a multiple of tp and at least 256
  int parity = 0;

  unsigned m;
  {
    const unsigned lim1[1] = {range + 1u};
    unsigned c1[1];
    sr_count<1>(mine, steps, lim1, c1);
    sr_combine<1>(part, parity, t, px, tp, slices, c1);
    m = c1[0];
  }
  unsigned k[NQ], ans[NQ], lim[NQ], c[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    k[i] = m ? (unsigned)qs.q[i] * (m - 1u) / 1000u : 0u;  // rank_of, the host's rule
    ans[i] = 0u;
  }
  for (unsigned bit = 0x8000u; bit; bit >>= 1) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const unsigned cand = ans[i] | bit;
      lim[i] = cand < range + 1u ? cand : range + 1u;
    }
    sr_count<NQ>(mine, steps, lim, c);
    sr_combine<NQ>(part, parity, t, px, tp, slices, c);
#pragma unroll
    for (int i = 0; i < NQ; ++i)
      if (c[i] <= k[i]) ans[i] |= bit;
  }

  if (t < tp && px < np) {  // slice 0 stores
#pragma unroll
    for (int i = 0; i < NQ; ++i) out[(size_t)i * P + p0 + (size_t)px] = (uint16_t)(m ? ans[i] + lo : 0u);
    if (valid) valid[p0 + (size_t)px] = (uint16_t)m;
  }
}

}  // namespace sr
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_STACKRANK_H */
