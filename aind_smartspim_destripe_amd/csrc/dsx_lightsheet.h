// dsx_lightsheet.h -- light-sheet background mode: two windowed percentile (rank) filters per plane and the subtraction
// of the background they estimate (gfx950), and the host build of the same arithmetic (dsx_lightsheet_ref).
//
// Contract (DESIGN.md "Light-sheet background mode"), per uint16 plane x[H, W], stripes along x:
//   q      = floor(255 log2(1 + x) / 16), exact through the 255 integer edges E[v] = smallest x with q(x) >= v
//   P(h,w) = skimage.filters.rank.percentile(q, ones((h, w)), p0 = p): window rows i - h/2 .. i - h/2 + h - 1, columns
//            j - w/2 .. j - w/2 + w - 1, only the n pixels inside the plane counted, result the smallest v with
//            #{q <= v in the window} >= floor(p n) + 1  (p n in float64)
//   ls = P(1, A), bg = P(B, B);  L = Bk[ls], G = Bk[bg];  offset = L <= float32(lambda) G ? L : G
//   out = max(float32(x) - offset, 0)                      (float32, or uint16 by truncation)
// E and Bk come from the caller (Python makes them in float64), so nothing here evaluates a logarithm.
//
// Kernels (launched in this order by dsx.hip, one launch each per cohort):
//   k_ls_quant : q, one thread per pixel, an 8-step binary search over E held in LDS.
//   k_ls_row<CT, T> : the 1 x A filter, Huang's sliding histogram.  A thread owns a run of kLsRun output pixels of one
//       row and a private 256-bin histogram in LDS (counts CT: bytes while A <= 255, 16 bits above), padded by one
//       word per thread so that equal bins of neighbouring threads fall into different banks.  It fills the window of
//       its first pixel, then per pixel removes the leaving value, adds the entering one and walks the percentile bin
//       up or down (`below` = pixels under the bin), so a step costs a few LDS operations whatever A is.
//   k_ls_bg<TO> : the B x B filter (Perreault's column histograms) and the subtraction.  A block of 8 waves owns a strip
//       of S = kLsCols - (B - 1) output columns and kLsRows rows of one plane.  LDS holds one 256-bin histogram per
//       column the strip's windows touch (S + B - 1 columns).  A column never holds more than B <= 255 pixels, so its
//       counts are BYTES: 256 B per column, 600 columns in 156 KB, where 16-bit counts would leave no strip at all at
//       B = 255.  (The window's counts reach B^2 and live in registers.)  Columns are 65 words apart: equal bins of
//       neighbouring columns and the 64 words of one column both spread over all banks.  Marching down the rows each
//       thread adds the entering and removes the leaving pixel of its own columns; columns outside the plane stay
//       empty, which IS the border rule (nothing padded, n shrinks), n itself is computed from the geometry.  Each wave
//       then slides a window histogram over an eighth of the strip: lane l holds bins 4l .. 4l+3 as two packed pairs of
//       16-bit counts (<= 65 025), one step is two conflict-free word reads (entering, leaving column), four packed
//       adds, a DPP prefix sum over the wave and a ballot for the first lane that reaches the rank.  Results are kept
//       one per lane and every 64 steps the wave stores 64 bg values and the 64 finished pixels (step 3) coalesced.
//   No global atomics; no per-thread arrays (histograms are in LDS), so no scratch.
#ifndef DSX_LIGHTSHEET_H
#define DSX_LIGHTSHEET_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define DSX_LS_HD __host__ __device__ __forceinline__
#else
#define DSX_LS_HD inline
#endif

namespace dsx {
namespace ls {

constexpr int kLsEdges = 255;   // E[1] .. E[255], stored at index v - 1
constexpr int kLsMaxA = 1024;   // artifact_length
constexpr int kLsMaxB = 255;    // background_window_size: B^2 fits a 16-bit count
constexpr int kLsRun = 64;      // k_ls_row: output pixels per thread (a row is split into runs of this length)
constexpr int kLsRows = 32;     // k_ls_bg: rows per block
constexpr int kLsCols = 600;    // k_ls_bg: column histograms per block (600 x 260 B = 156 000 B of the CU's 160 KiB)
constexpr int kLsColWords = 65; // words between two column histograms (64 of counts and one of padding)
constexpr int kLsBgThreads = 512;  // k_ls_bg: eight waves share a strip, two per SIMD
constexpr int kLsBgWaves = kLsBgThreads / 64;

// output columns of a k_ls_bg strip for window size B
inline int bg_strip(int B) { return kLsCols - (B - 1); }

// dynamic LDS of a k_ls_bg block: 256 words of the back table and (min(S, W) + B - 1) column histograms
inline size_t bg_lds_bytes(int W, int B) {
  const int S = bg_strip(B);
  return ((size_t)256 + (size_t)((S < W ? S : W) + B - 1) * kLsColWords) * 4;
}

// q(x): the number of edges E[v] <= x, E non-decreasing
DSX_LS_HD int ls_quant(const uint32_t* E, uint32_t x) {
  int lo = 0, hi = kLsEdges;  // answer in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (E[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the rank the percentile bin has to reach: floor(p n) + 1 with p n in float64 (never above n)
DSX_LS_HD int ls_rank(double p, int n) {
  const int t = (int)(p * (double)n) + 1;
  return t < n ? t : n;
}

// pixels of a window of `len` starting at `first` that lie in [0, size)
DSX_LS_HD int ls_inside(int first, int len, int size) {
  const int a = first > 0 ? first : 0, b = first + len < size ? first + len : size;
  return b - a;
}

// step 3 for one pixel: every operation a single float32 one
DSX_LS_HD float ls_subtract(uint16_t x, float L, float G, float lam) {
  const float bound = lam * G;
  const float offset = L <= bound ? L : G;
  const float d = (float)x - offset;
  return d > 0.f ? d : 0.f;
}

// the argument rules of dsx_plan_lightsheet / dsx_lightsheet_ref: the message of the first one broken, or nullptr
inline const char* lightsheet_args(int H, int W, double p, int A, int B, double lambda, const uint32_t* E,
                                   const float* back) {
  if (H < 1 || W < 1) return "plane must be at least 1 x 1";
  if (!(p > 0.0 && p < 1.0)) return "lightsheet: percentile must lie in (0, 1)";
  if (A < 1 || A > kLsMaxA) return "lightsheet: artifact_length must be in 1 .. 1024";
  if (B < 1 || B > kLsMaxB) return "lightsheet: background_window_size must be in 1 .. 255";
  if (!(lambda > 0.0) || !((float)lambda > 0.f) || !((float)lambda < 3.0e38f))
    return "lightsheet: lightsheet_vs_background must be positive and finite";
  if (!E || !back) return "lightsheet: the edge table or the back table is NULL";
  for (int v = 1; v < kLsEdges; ++v)
    if (E[v] < E[v - 1]) return "lightsheet: the edge table must not decrease";
  return nullptr;
}

// ---- host build ------------------------------------------------------------------------------------------------
inline void quant_host(const uint16_t* x, size_t n, const uint32_t* E, uint8_t* q) {
  std::vector<uint8_t> lut(65536);
  for (uint32_t v = 0; v < 65536u; ++v) lut[v] = (uint8_t)ls_quant(E, v);
  for (size_t i = 0; i < n; ++i) q[i] = lut[x[i]];
}

// P(q; h, w) over one plane: column histograms of the h rows around the current row, a window histogram slid along it
inline void percentile_host(const uint8_t* q, int H, int W, int h, int w, double p, uint8_t* out) {
  std::vector<uint16_t> col((size_t)W * 256, 0);
  std::vector<int> win(256);
  const int hh = h / 2, hw = w / 2;
  for (int r = 0; r < h - hh && r < H; ++r)  // rows of the window of row 0: -hh .. h - hh - 1
    for (int c = 0; c < W; ++c) ++col[(size_t)c * 256 + q[(size_t)r * W + c]];
  for (int i = 0; i < H; ++i) {
    if (i > 0) {
      const int leave = i - 1 - hh, enter = i - hh + h - 1;
      if (leave >= 0)
        for (int c = 0; c < W; ++c) --col[(size_t)c * 256 + q[(size_t)leave * W + c]];
      if (enter < H)
        for (int c = 0; c < W; ++c) ++col[(size_t)c * 256 + q[(size_t)enter * W + c]];
    }
    const int rows_in = ls_inside(i - hh, h, H);
    for (int b = 0; b < 256; ++b) win[b] = 0;
    for (int c = 0; c < w - hw && c < W; ++c)
      for (int b = 0; b < 256; ++b) win[b] += col[(size_t)c * 256 + b];
    for (int j = 0; j < W; ++j) {
      if (j > 0) {
        const int leave = j - 1 - hw, enter = j - hw + w - 1;
        if (leave >= 0)
          for (int b = 0; b < 256; ++b) win[b] -= col[(size_t)leave * 256 + b];
        if (enter < W)
          for (int b = 0; b < 256; ++b) win[b] += col[(size_t)enter * 256 + b];
      }
      const int t = ls_rank(p, rows_in * ls_inside(j - hw, w, W));
      int v = 0, sum = win[0];
      while (sum < t) sum += win[++v];
      out[(size_t)i * W + j] = (uint8_t)v;
    }
  }
}

// one plane through all three steps; q, lsp, bgp: [H][W] planes the caller provides
template <typename TO>
void lightsheet_host(const uint16_t* x, int H, int W, double p, int A, int B, float lam, const uint32_t* E,
                     const float* back, uint8_t* q, uint8_t* lsp, uint8_t* bgp, TO* out) {
  const size_t n = (size_t)H * W;
  quant_host(x, n, E, q);
  percentile_host(q, H, W, 1, A, p, lsp);
  percentile_host(q, H, W, B, B, p, bgp);
  for (size_t i = 0; i < n; ++i) out[i] = (TO)ls_subtract(x[i], back[lsp[i]], back[bgp[i]], lam);
}

}  // namespace ls
}  // namespace dsx

#if defined(__HIP__)

namespace dsx {
namespace ls {

__global__ __launch_bounds__(256) void k_ls_quant(const uint16_t* __restrict__ x, size_t n,
                                                   const uint32_t* __restrict__ edges, uint8_t* __restrict__ q) {
  __shared__ uint32_t E[256];
  if (threadIdx.x < kLsEdges) E[threadIdx.x] = edges[threadIdx.x];
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) q[i] = (uint8_t)ls_quant(E, x[i]);
}

// grid: ceil(planes * H * ceil(W / kLsRun) / T) blocks of T threads; q, out: [planes][H][W]
template <typename CT, int T>
__global__ __launch_bounds__(T) void k_ls_row(const uint8_t* __restrict__ q, uint8_t* __restrict__ out, size_t rows,
                                              int W, int A, double p) {
  constexpr int kWords = 256 * (int)sizeof(CT) / 4 + 1;  // histogram of a thread, padded by one word
  __shared__ uint32_t smem[T * kWords];
  const int rpr = (W + kLsRun - 1) / kLsRun;
  const size_t g = (size_t)blockIdx.x * T + threadIdx.x;
  if (g >= rows * (size_t)rpr) return;  // (no barrier below)
  const size_t row = g / rpr;
  const int j0 = (int)(g - row * rpr) * kLsRun, j1 = j0 + kLsRun < W ? j0 + kLsRun : W;
  const uint8_t* qr = q + row * W;
  uint8_t* o = out + row * W;
  uint32_t* words = smem + threadIdx.x * kWords;
  for (int k = 0; k < kWords; ++k) words[k] = 0u;
  CT* hist = reinterpret_cast<CT*>(words);

  const int half = A / 2;
  int lo = j0 - half, hi = j0 - half + A;  // window of j0: [lo, hi) cut to the row
  lo = lo > 0 ? lo : 0;
  hi = hi < W ? hi : W;
  for (int c = lo; c < hi; ++c) ++hist[qr[c]];
  int n = hi - lo, v = 0, below = 0;
  for (int j = j0; j < j1; ++j) {
    if (j > j0) {
      const int leave = j - 1 - half, enter = j - half + A - 1;
      if (leave >= 0) {
        const int r = qr[leave];
        --hist[r];
        --n;
        below -= r < v;
      }
      if (enter < W) {
        const int a = qr[enter];
        ++hist[a];
        ++n;
        below += a < v;
      }
    }
    const int t = ls_rank(p, n);
    while (below >= t) below -= hist[--v];
    for (int c = hist[v]; below + c < t; c = hist[v]) {
      below += c;
      ++v;
    }
    o[j] = (uint8_t)v;
  }
}

// inclusive prefix sum over the 64 lanes (DPP: shifts inside the rows of 16, then the two row broadcasts)
__device__ __forceinline__ int wave_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
  return v;
}

// grid: (strips of S columns, segments of kLsRows rows, planes); block: kLsBgThreads; dynamic LDS: bg_lds_bytes(W, B).  x, q, lsp, bgp, out: [planes][H][W].
template <typename TO>
__global__ __launch_bounds__(kLsBgThreads) void k_ls_bg(const uint16_t* __restrict__ x, const uint8_t* __restrict__ q,
                                                         const uint8_t* __restrict__ lsp, uint8_t* __restrict__ bgp,
                                                         TO* __restrict__ out, const float* __restrict__ back, int H,
                                                         int W, int B, int S, double p, float lam) {
  extern __shared__ uint32_t lds[];  // the back table, then the column histograms (one allocation: the raised limit
  float* Bk = reinterpret_cast<float*>(lds);  // of 160 KiB covers dynamic and static LDS together)
  uint32_t* colw = lds + 256;
  uint8_t* colb = reinterpret_cast<uint8_t*>(colw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = B / 2;
  const int c0 = blockIdx.x * S, Sb = S < W - c0 ? S : W - c0;
  const int i0 = blockIdx.y * kLsRows, i1 = i0 + kLsRows < H ? i0 + kLsRows : H;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const uint8_t* qp = q + plane;
  const int ncol = Sb + B - 1, cbase = c0 - half;  // LDS column k is plane column cbase + k

  if (tid < 256) Bk[tid] = back[tid];
  for (int k = tid; k < ncol * kLsColWords; k += kLsBgThreads) colw[k] = 0u;
  __syncthreads();
  // a thread keeps to its own columns from here on, so the row updates need no barrier among themselves
  {
    const int r0 = i0 - half > 0 ? i0 - half : 0, r1 = i0 - half + B < H ? i0 - half + B : H;
    for (int k = tid; k < ncol; k += kLsBgThreads) {
      const int c = cbase + k;
      if (c < 0 || c >= W) continue;
      for (int r = r0; r < r1; ++r) ++colb[k * (kLsColWords * 4) + qp[(size_t)r * W + c]];
    }
  }
  __syncthreads();

  const int chunk = (Sb + kLsBgWaves - 1) / kLsBgWaves;
  const int ja = c0 + wave * chunk, jb = ja + chunk < c0 + Sb ? ja + chunk : c0 + Sb;
  for (int i = i0; i < i1; ++i) {
    if (i > i0) {
      const int leave = i - 1 - half, enter = i - half + B - 1;
      for (int k = tid; k < ncol; k += kLsBgThreads) {
        const int c = cbase + k;
        if (c < 0 || c >= W) continue;
        if (leave >= 0) --colb[k * (kLsColWords * 4) + qp[(size_t)leave * W + c]];
        if (enter < H) ++colb[k * (kLsColWords * 4) + qp[(size_t)enter * W + c]];
      }
      __syncthreads();
    }
    if (ja < jb) {
      const int rows_in = ls_inside(i - half, B, H);
      // window of ja: LDS columns ja - c0 .. ja - c0 + B - 1; lane l: bins 4l, 4l+2 in h02 and 4l+1, 4l+3 in h13
      uint32_t h02 = 0u, h13 = 0u;
      const uint32_t* cw = colw + (ja - c0) * kLsColWords + lane;
      for (int k = 0; k < B; ++k) {
        const uint32_t d = cw[k * kLsColWords];
        h02 += d & 0x00ff00ffu;
        h13 += (d >> 8) & 0x00ff00ffu;
      }
      int keep = 0;
      for (int j = ja; j < jb; ++j) {
        const int t = ls_rank(p, rows_in * ls_inside(j - half, B, W));
        const uint32_t pair = h02 + h13;  // bins 4l + 4l+1 | 4l+2 + 4l+3: the whole window is at most 65 025
        const int s = (int)((pair & 0xffffu) + (pair >> 16));
        const int incl = wave_scan(s);
        const unsigned long long reach = __ballot(incl >= t);
        const int first = __builtin_amdgcn_readfirstlane(reach ? (int)__builtin_ctzll(reach) : 63);
        int e = incl - s;  // pixels below this lane's bins
        int mine = 4 * lane;
        e += (int)(h02 & 0xffffu); mine += e < t;
        e += (int)(h13 & 0xffffu); mine += e < t;
        e += (int)(h02 >> 16); mine += e < t;
        const int res = __builtin_amdgcn_readlane(mine, first);
        const int step = (j - ja) & 63;
        if (lane == step) keep = res;
        if (step == 63 || j == jb - 1) {  // 64 results (or the rest of the chunk): bg and the finished pixels
          if (lane <= step) {
            const size_t idx = plane + (size_t)i * W + (j - step + lane);
            bgp[idx] = (uint8_t)keep;
            out[idx] = (TO)ls_subtract(x[idx], Bk[lsp[idx]], Bk[keep], lam);
          }
        }
        if (j + 1 < jb) {  // column j - half leaves, column j - half + B enters
          const uint32_t dl = cw[(j - ja) * kLsColWords], de = cw[(j - ja + B) * kLsColWords];
          h02 += (de & 0x00ff00ffu) - (dl & 0x00ff00ffu);
          h13 += ((de >> 8) & 0x00ff00ffu) - ((dl >> 8) & 0x00ff00ffu);
        }
      }
    }
    __syncthreads();  // the next row's update changes the columns this row's windows read
  }
}

}  // namespace ls
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_LIGHTSHEET_H */
