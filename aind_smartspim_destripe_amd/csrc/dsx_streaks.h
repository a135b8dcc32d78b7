// dsx_streaks.h -- kernels of the dual-band wavelet-FFT stripe filter (filter_streaks with sigma = (fg, bg)).
//
// The filter (README "filter_streaks", the upstream pystripe form with the reference's own helpers):
//   t      per-plane Otsu threshold of the input (skimage threshold_otsu: one bin per integer for uint16,
//          256 NumPy bins for float32), or a fixed value
//   band   y = log(1 + z) of the edge-padded even plane, wavedec2 (mode symmetric), every cH row filtered with
//          irfft(rfft(cH) * notch), waverec2, exp(r) - 1
//   blend  b = band(min(x, t), sigma_bg), f = band(max(x, t), sigma_fg), w = sigmoid((x - t) / crossover),
//          out = f w + b (1 - w); a single band (sigma_fg == sigma_bg) is band(x, sigma_fg)
//
// Layout: the P = bands * nb "virtual planes" of a cohort of nb planes are band-major (v = band * nb + plane), so the
// cH rows of one band are contiguous and one row-filter launch covers them.  Every kernel maps one thread to one
// output element and checks it against the element count; none uses scratch memory.
//
//   k_st_minmax   per-plane min / max (order-preserving uint keys, atomics)
//   k_st_hist     per-plane histogram: uint16 one bin per integer of [min, max] (<= 65536 bins, counted in LDS
//                 windows of kStWin bins, flushed to global memory); float32 the 256 bins of numpy.histogram
//   k_st_otsu     class-variance arg-max in float64, first maximum (skimage); one block per plane
//   k_st_prep     log(1 + min(x, t)) and log(1 + max(x, t)) (or log(1 + x)) of the edge-padded plane
//   k_st_dwt<A>   one analysis pass along axis A (lo and hi outputs)
//   k_st_rowmat   the row filter as two thin products per level and band: Z = cH U (n x K), cH' = cH + Z V (K x n),
//                 the low-rank form of irfft(rfft(cH) * g) - cH (only K ~ 6.4 s packed gains differ from 1)
//   k_st_idwt<A>  one synthesis pass along axis A
//   k_st_final    exp(r) - 1 per band, sigmoid blend, crop, float32 / uint16 store
//
// March route (dsx_plan_streaks_ex, DSX_STREAKS_MARCH): the bands go through the log-space chain of dsx.hip instead of
// k_st_prep ... k_st_idwt; t comes from the same k_st_minmax / k_st_hist / k_st_otsu / k_st_fill.
//   k_st_chainfill  what the chain's row filters read per virtual plane: mask threshold +inf on every level, cfg = band
//   k_st_bands      the virtual input planes max(x, t) (2k) and min(x, t) (2k + 1), or x for a single band
//   k_st_blend      (F - 2) w + (B - 2) (1 - w) of the chain's float32 planes, float32 / uint16 store
//
// Options (dsx_plan_streaks_opts: one-sided bands, a smoothed blend weight, dark / flat): k_st_blendx replaces k_st_final
// and k_st_blend, on either route, when an option is set; with none set those two run as before.
//   k_st_blendx     one body over a band-loader policy (StGenericBands: expm1 of the band-major [P][Hp][Wp] planes,
//                   StMarchBands: r - 2 of the virtual planes); a block owns a 64 x 16 output tile, evaluates the
//                   sigmoid of tile + halo into LDS once, smooths it there in two 1-D passes, blends, applies
//                   flatfield_correction and stores float32 / uint16
//   st_blend_host   the same weight, fold, tap, blend and epilogue functions over one plane on the host
//                   (dsx_streaks_blend_ref)
#ifndef DSX_STREAKS_H
#define DSX_STREAKS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dsx_wavelet.h"

namespace dsx {
namespace st {

constexpr int kStWin = 8192;    // uint16 histogram bins per LDS window (32 KiB)
constexpr int kStBins = 65536;  // global histogram capacity per plane
constexpr int kOtsuThreads = 1024;
// which bands a plan filters (DSX_STREAKS_BANDS_*); kStSingle: equal sigmas, one band of the unclipped plane, no weight
enum { kStBoth = 0, kStFg = 1, kStBg = 2, kStSingle = 3 };
#define DSX_ST_HD __host__ __device__ __forceinline__

struct Taps {
  float lo[kMaxTaps], hi[kMaxTaps];  // kMaxTaps: dsx_wavelet.h, the bound dsx_set_wavelet enforces
};

// (order-preserving integer keys of floats: dsx::f32_key / dsx::key_f32, dsx_kernels.h)

template <typename T>
__device__ __forceinline__ float pix(const T* p, size_t i) { return (float)p[i]; }

// mm[2 b] = min key, mm[2 b + 1] = max key (uint16: the value itself); grid (blocks, planes)
template <typename T>
__global__ __launch_bounds__(256) void k_st_minmax(const T* __restrict__ in, size_t plane_px, unsigned* mm) {
  const T* p = in + (size_t)blockIdx.y * plane_px;
  unsigned lo = 0xffffffffu, hi = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane_px; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned k = sizeof(T) == 2 ? (unsigned)p[i] : f32_key(pix(p, i));
    lo = min(lo, k);
    hi = max(hi, k);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(mm + 2 * blockIdx.y, lo);
    atomicMax(mm + 2 * blockIdx.y + 1, hi);
  }
}

// numpy.histogram(x, bins=256) edges of NumPy 1.26: float64 arange(257) * ((last - first) / 256) + first, last edge
// exact, rounded to float32 (oracle.destripe_oracle.histogram256); no contraction into fma
__device__ __forceinline__ void f32_range(const unsigned* mm, float& first, float& last) {
  first = key_f32(mm[0]);
  last = key_f32(mm[1]);
  if (first == last) { first -= 0.5f; last += 0.5f; }
}
__device__ __forceinline__ float f32_edge(float first, float last, int k) {
  if (k >= 256) return last;
  const double step = __ddiv_rn(__dsub_rn((double)last, (double)first), 256.0);
  return (float)__dadd_rn(__dmul_rn((double)k, step), (double)first);
}

// grid (blocks, planes); hist[b * kStBins + k]
template <typename T>
__global__ __launch_bounds__(256) void k_st_hist(const T* __restrict__ in, size_t plane_px, const unsigned* mm,
                                                 unsigned* hist) {
  __shared__ unsigned h[kStWin];
  __shared__ float edges[257];
  const T* p = in + (size_t)blockIdx.y * plane_px;
  unsigned* gh = hist + (size_t)blockIdx.y * kStBins;
  const size_t start = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (sizeof(T) == 2) {
    const unsigned vmin = mm[2 * blockIdx.y], vmax = mm[2 * blockIdx.y + 1];
    const unsigned nbins = vmax - vmin + 1;
    for (unsigned base = 0; base < nbins; base += kStWin) {
      for (int k = threadIdx.x; k < kStWin; k += blockDim.x) h[k] = 0u;
      __syncthreads();
      for (size_t i = start; i < plane_px; i += step) {
        const unsigned k = (unsigned)p[i] - vmin - base;
        if (k < (unsigned)kStWin) atomicAdd(&h[k], 1u);
      }
      __syncthreads();
      for (int k = threadIdx.x; k < kStWin && base + k < nbins; k += blockDim.x)
        if (h[k]) atomicAdd(gh + base + k, h[k]);
      __syncthreads();
    }
  } else {
    float first, last;
    f32_range(mm + 2 * blockIdx.y, first, last);
    for (int k = threadIdx.x; k < 257; k += blockDim.x) edges[k] = f32_edge(first, last, k);
    for (int k = threadIdx.x; k < 256; k += blockDim.x) h[k] = 0u;
    __syncthreads();
    const float denom = last - first;
    for (size_t i = start; i < plane_px; i += step) {
      const float a = pix(p, i);
      int idx = (int)(__fmul_rn(__fdiv_rn(__fsub_rn(a, first), denom), 256.0f));
      idx = min(max(idx, 0), 256);
      if (idx == 256) idx = 255;
      if (a < edges[idx]) idx -= 1;
      if (idx < 0) idx = 0;
      if (a >= edges[idx + 1] && idx != 255) idx += 1;
      atomicAdd(&h[idx], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 256; k += blockDim.x)
      if (h[k]) atomicAdd(gh + k, h[k]);
  }
}

// skimage threshold_otsu on the histogram: first arg-max of w1[i] w2[i+1] (m1[i] - m2[i+1])^2, i < nbins - 1, in
// float64.  uint16: bin centres min + k (every sum an exact integer, so the curve is skimage's to the bit);
// float32: centres (e[k] + e[k+1]) / 2 in float32.  A constant plane returns its value.  One block per plane.
struct OtsuOut {
  double t;
  int bin;
  int nbins;
};

template <bool U16>
__device__ __forceinline__ double bin_centre(int k, unsigned vmin, float first, float last) {
  if (U16) return (double)(vmin + (unsigned)k);
  return (double)((f32_edge(first, last, k) + f32_edge(first, last, k + 1)) * 0.5f);
}

template <bool U16>
__global__ __launch_bounds__(kOtsuThreads) void k_st_otsu(const unsigned* mm, const unsigned* hist, float* t_out,
                                                         OtsuOut* info) {
  __shared__ unsigned long long sw[kOtsuThreads];
  __shared__ double ss[kOtsuThreads];
  __shared__ double bv[kOtsuThreads];
  __shared__ int bi[kOtsuThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned* h = hist + (size_t)b * kStBins;
  const unsigned vmin = mm[2 * b], vmax = mm[2 * b + 1];
  float first = 0.f, last = 0.f;
  int nbins;
  if (U16) {
    nbins = (int)(vmax - vmin + 1);
  } else {
    f32_range(mm + 2 * b, first, last);
    nbins = 256;
  }
  const bool constant = vmin == vmax;
  if (constant) {
    if (tid == 0) {
      const double v = U16 ? (double)vmin : (double)key_f32(vmin);
      t_out[b] = (float)v;
      info[b].t = v;
      info[b].bin = 0;
      info[b].nbins = 1;
    }
    return;
  }
  const int per = (nbins + kOtsuThreads - 1) / kOtsuThreads;
  const int k0 = min(tid * per, nbins), k1 = min(k0 + per, nbins);
  unsigned long long w = 0;
  double s = 0.0;
  for (int k = k0; k < k1; ++k) {
    w += h[k];
    s += (double)h[k] * bin_centre<U16>(k, vmin, first, last);
  }
  sw[tid] = w;
  ss[tid] = s;
  __syncthreads();
  // inclusive scan (Hillis-Steele) of the per-thread sums
  for (int o = 1; o < kOtsuThreads; o <<= 1) {
    const unsigned long long aw = tid >= o ? sw[tid - o] : 0ull;
    const double as = tid >= o ? ss[tid - o] : 0.0;
    __syncthreads();
    sw[tid] += aw;
    ss[tid] += as;
    __syncthreads();
  }
  const unsigned long long wtot = sw[kOtsuThreads - 1];
  const double stot = ss[kOtsuThreads - 1];
  unsigned long long w1 = tid ? sw[tid - 1] : 0ull;
  double s1 = tid ? ss[tid - 1] : 0.0;
  double best = -1.0;
  int besti = 0x7fffffff;
  for (int k = k0; k < k1 && k < nbins - 1; ++k) {
    w1 += h[k];
    s1 += (double)h[k] * bin_centre<U16>(k, vmin, first, last);
    const unsigned long long w2 = wtot - w1;
    const double m1 = s1 / (double)w1, m2 = (stot - s1) / (double)w2;
    const double d = m1 - m2;
    const double v = (double)(w1 * w2) * (d * d);
    if (v > best) { best = v; besti = k; }
  }
  bv[tid] = best;
  bi[tid] = besti;
  __syncthreads();
  for (int o = kOtsuThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double v2 = bv[tid + o];
      const int i2 = bi[tid + o];
      if (v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid])) { bv[tid] = v2; bi[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int k = bi[0] == 0x7fffffff ? 0 : bi[0];
    const double t = bin_centre<U16>(k, vmin, first, last);
    t_out[b] = (float)t;
    info[b].t = t;
    info[b].bin = k;
    info[b].nbins = nbins;
  }
}

__global__ __launch_bounds__(256) void k_st_fill(float* t, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) t[i] = v;
}

// y[v][i][j], v = band * B + b: log(1 + min(x, t)) (band 0), log(1 + max(x, t)) (band 1), or log(1 + x) for a
// single band; x of the plane edge-padded to Hp x Wp (last row / column repeated).  clip (one band only): kStFg the
// band is max(x, t), kStBg it is min(x, t) -- a one-sided plan writes only the band it filters
template <typename T>
__global__ __launch_bounds__(256) void k_st_prep(const T* __restrict__ in, int nb, int B, int H, int W, int Hp, int Wp,
                                                 int bands, int clip, const float* t, float* y, unsigned* sticky) {
  const size_t per = (size_t)Hp * Wp, total = per * nb * bands;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % Wp);
  const int i = (int)((idx / Wp) % Hp);
  const int b = (int)((idx / per) % nb);
  const int band = (int)(idx / (per * nb));
  const float x = pix(in, (size_t)b * H * W + (size_t)min(i, H - 1) * W + min(j, W - 1));
  // a float32 pixel that is NaN, infinite or <= -1 has no finite log(1 + x): the reference's threshold_otsu raises
  // ValueError for such a plane; flag it in the context's host-mapped word (read by dsx_run_host / dsx_sync)
  if (sizeof(T) == 4 && band == 0 && !(x > -1.0f && x < INFINITY) && sticky != nullptr) *(volatile unsigned*)sticky = 1u;
  float z = x;
  if (bands == 2) z = band == 0 ? fminf(x, t[b]) : fmaxf(x, t[b]);
  else if (clip == kStFg) z = fmaxf(x, t[b]);
  else if (clip == kStBg) z = fminf(x, t[b]);
  y[((size_t)band * B + b) * per + (size_t)i * Wp + j] = logf(1.0f + z);
}

DSX_ST_HD int st_refl(int i, int n) {  // half-sample symmetric extension, any distance
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// one analysis pass along axis A of [P][h][w] planes (row pitch ld_in); lo / hi [P][ho][wo] dense
template <int A>
__global__ __launch_bounds__(256) void k_st_dwt(const float* __restrict__ x, int P, int h, int w, int ld_in,
                                                size_t ps_in, float* lo, float* hi, int F, Taps tp) {
  const int n = A == 0 ? h : w;
  const int m = (n + F - 1) / 2;
  const int ho = A == 0 ? m : h, wo = A == 0 ? w : m;
  const size_t per = (size_t)ho * wo, total = per * P;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % wo), r = (int)((idx / wo) % ho), v = (int)(idx / per);
  const float* src = x + (size_t)v * ps_in;
  const int o = A == 0 ? r : c;
  float sl = 0.f, sh = 0.f;
  for (int k = 0; k < F; ++k) {
    const int q = st_refl(2 * o + 1 - k, n);
    const float xv = A == 0 ? src[(size_t)q * ld_in + c] : src[(size_t)r * ld_in + q];
    sl = fmaf(tp.lo[k], xv, sl);
    sh = fmaf(tp.hi[k], xv, sh);
  }
  lo[idx] = sl;
  hi[idx] = sh;
}

// one synthesis pass along axis A: a [P][h][w] (pitch lda, plane stride psa) and d (pitch ldd, stride psd), both read
// over the h x w of d (a may be one longer: waverec2 trims it); out [P][ho][wo] with pitch wo, n_out = 2 m - F + 2
template <int A>
__global__ __launch_bounds__(256) void k_st_idwt(const float* __restrict__ a, int lda, size_t psa,
                                                 const float* __restrict__ d, int ldd, size_t psd, int P, int h, int w,
                                                 float* out, int F, Taps tp) {
  const int m = A == 0 ? h : w;
  const int no = 2 * m - F + 2;
  const int ho = A == 0 ? no : h, wo = A == 0 ? w : no;
  const size_t per = (size_t)ho * wo, total = per * P;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % wo), r = (int)((idx / wo) % ho), v = (int)(idx / per);
  const float* sa = a + (size_t)v * psa;
  const float* sd = d + (size_t)v * psd;
  const int nn = A == 0 ? r : c;
  const int p = nn >> 1, bit = nn & 1;
  float s = 0.f;
  for (int j = 0; j < F / 2; ++j) {
    const int tix = F - 2 - 2 * j + bit;
    const size_t ia = A == 0 ? (size_t)(p + j) * lda + c : (size_t)r * lda + (p + j);
    const size_t id = A == 0 ? (size_t)(p + j) * ldd + c : (size_t)r * ldd + (p + j);
    s = fmaf(sa[ia], tp.lo[tix], s);
    s = fmaf(sd[id], tp.hi[tix], s);
  }
  out[idx] = s;
}

// C[R][N] = X[R][Kd] M[Kd][N] (+ E[R][N] when E is given), all row-major and dense; 64 x 64 tiles, 4 x 4 results per
// thread.  E may alias nothing else (C != X, C != E).
constexpr int kMmT = 64, kMmK = 16;
__global__ __launch_bounds__(256) void k_st_rowmat(const float* __restrict__ X, const float* __restrict__ M,
                                                   const float* __restrict__ E, float* __restrict__ C, int R, int Kd,
                                                   int N) {
  __shared__ float xs[kMmK][kMmT + 4];
  __shared__ float ms[kMmK][kMmT + 4];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int row0 = blockIdx.y * kMmT, col0 = blockIdx.x * kMmT;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < Kd; k0 += kMmK) {
    for (int e = threadIdx.x; e < kMmT * kMmK; e += 256) {
      const int rr = e / kMmK, kk = e % kMmK;  // X tile: 64 rows x 16 k
      const int gr = row0 + rr, gk = k0 + kk;
      xs[kk][rr] = (gr < R && gk < Kd) ? X[(size_t)gr * Kd + gk] : 0.f;
      const int mk = e / kMmT, mc = e % kMmT;  // M tile: 16 k x 64 cols
      const int gk2 = k0 + mk, gc = col0 + mc;
      ms[mk][mc] = (gk2 < Kd && gc < N) ? M[(size_t)gk2 * N + gc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kMmK; ++kk) {
      float xa[4], mb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xa[q] = xs[kk][ty + 16 * q];
        mb[q] = ms[kk][tx + 16 * q];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xa[i], mb[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = row0 + ty + 16 * i;
    if (gr >= R) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = col0 + tx + 16 * j;
      if (gc < N) C[(size_t)gr * N + gc] = E ? E[(size_t)gr * N + gc] + acc[i][j] : acc[i][j];
    }
  }
}

// w of the blend: the reference's foreground_fraction(x, t, crossover)
DSX_ST_HD float st_weight(float x, float t, float inv_crossover) {
  return 1.0f / (1.0f + expf(-(x - t) * inv_crossover));
}

// out[b][i][j], i < H, j < W: exp(r) - 1 per band (r: [P][Hp][Wp], band-major), blend, store
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void k_st_final(const TI* __restrict__ in, const float* __restrict__ r, int nb, int B,
                                                  int H, int W, int Hp, int Wp, int bands, const float* t,
                                                  float inv_crossover, TO* out) {
  const size_t per = (size_t)H * W, total = per * nb;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % W), i = (int)((idx / W) % H), b = (int)(idx / per);
  const size_t pp = (size_t)Hp * Wp, off = (size_t)i * Wp + j;
  float res;
  if (bands == 1) {
    res = expm1f(r[(size_t)b * pp + off]);
  } else {
    const float bg = expm1f(r[(size_t)b * pp + off]);
    const float fg = expm1f(r[((size_t)B + b) * pp + off]);
    const float x = pix(in, idx);
    const float wf = st_weight(x, t[b], inv_crossover);
    res = fg * wf + bg * (1.0f - wf);
  }
  if (sizeof(TO) == 2) {
    const float c = fminf(fmaxf(res, 0.0f), 65535.0f);
    out[idx] = (TO)(unsigned)c;
  } else {
    out[idx] = (TO)res;
  }
}

// ---- march route ---------------------------------------------------------------------------------------------------
// The virtual planes of real plane k are 2k (foreground band, cfg 0) and 2k + 1 (background band, cfg 1); a single band
// has one virtual plane per real plane (cfg 0).  Planes are H x W with H and W even (no padding), so a plane holds a
// multiple of 4 pixels: VEC = 4 moves 4 pixels per access where the caller's pointers allow it, VEC = 1 otherwise.
template <typename T, int N>
struct alignas(sizeof(T) * N) StVec {
  T v[N];
};

// one: the cfg of every plane when there is one band per real plane (1 for a background-only plan, else 0)
__global__ __launch_bounds__(256) void k_st_chainfill(float* thr, int n_thr, int* cfg, int n_cfg, int bands, int one) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_thr) thr[i] = INFINITY;
  if (i < n_cfg) cfg[i] = bands == 2 ? (i & 1) : one;
}

// grid (blocks, planes); v: [bands * planes][px].  clip (one band only): kStFg writes max(x, t), kStBg min(x, t)
template <typename TI, typename TV, int VEC>
__global__ __launch_bounds__(256) void k_st_bands(const TI* __restrict__ in, size_t px, int bands, int clip,
                                                  const float* t, TV* __restrict__ v, unsigned* sticky) {
  const int b = blockIdx.y;
  const float tb = t[b];
  const TI* p = in + (size_t)b * px;
  TV* f = v + (size_t)bands * b * px;
  TV* g = f + px;
  const size_t step = (size_t)gridDim.x * blockDim.x * VEC;
  bool bad = false;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < px; i += step) {
    const StVec<TI, VEC> x = *(const StVec<TI, VEC>*)(p + i);
    StVec<TV, VEC> hi, lo;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xv = (float)x.v[k];
      // as k_st_prep: a float32 pixel without a finite log(1 + x) flags the context's host-mapped word
      if (sizeof(TI) == 4 && !(xv > -1.0f && xv < INFINITY)) bad = true;
      hi.v[k] = (TV)(bands == 2 || clip == kStFg ? fmaxf(xv, tb) : clip == kStBg ? fminf(xv, tb) : xv);
      lo.v[k] = (TV)fminf(xv, tb);
    }
    *(StVec<TV, VEC>*)(f + i) = hi;
    if (bands == 2) *(StVec<TV, VEC>*)(g + i) = lo;
  }
  if (bad && sticky != nullptr) *(volatile unsigned*)sticky = 1u;
}

// grid (blocks, planes); r: [bands * planes][px], the chain's exp(.) + 1 of every band, i.e. band + 2
template <typename TI, typename TO, int VEC>
__global__ __launch_bounds__(256) void k_st_blend(const TI* __restrict__ in, const float* __restrict__ r, size_t px,
                                                  int bands, const float* t, float inv_crossover,
                                                  TO* __restrict__ out) {
  const int b = blockIdx.y;
  const float tb = t[b];
  const TI* p = in + (size_t)b * px;
  const float* f = r + (size_t)bands * b * px;
  const float* g = f + px;
  TO* o = out + (size_t)b * px;
  const size_t step = (size_t)gridDim.x * blockDim.x * VEC;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < px; i += step) {
    const StVec<float, VEC> fv = *(const StVec<float, VEC>*)(f + i);
    StVec<float, VEC> gv = fv;
    StVec<TI, VEC> x = {};
    if (bands == 2) {
      gv = *(const StVec<float, VEC>*)(g + i);
      x = *(const StVec<TI, VEC>*)(p + i);
    }
    StVec<TO, VEC> ov;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float res = fv.v[k] - 2.0f;
      if (bands == 2) {
        const float wf = st_weight((float)x.v[k], tb, inv_crossover);
        res = res * wf + (gv.v[k] - 2.0f) * (1.0f - wf);
      }
      if (sizeof(TO) == 2) ov.v[k] = (TO)(unsigned)fminf(fmaxf(res, 0.0f), 65535.0f);
      else ov.v[k] = (TO)res;
    }
    *(StVec<TO, VEC>*)(o + i) = ov;
  }
}

// ---- blend with options ---------------------------------------------------------------------------------------------
// w0 = st_weight(x) on the unpadded H x W plane; w = w0, or scipy.ndimage.gaussian_filter(w0, s) (separable, radius
// R = int(4 s + 0.5), taps exp(-k^2 / 2 s^2) normalised to sum 1, indices folded by st_refl); then
//   both bands f w + b (1 - w), foreground only f w + x (1 - w), background only x w + b (1 - w), single band f,
// and, with a flat, the reference's flatfield_correction(r, flat, dark).
constexpr int kStMaxR = 8;                      // s <= 2
constexpr int kBtW = 64, kBtH = 16;             // output tile of a block: 16 threads of 4 pixels across, 16 rows
constexpr int kBtPitch0 = kBtW + 2 * kStMaxR;   // row pitch of the sigmoid tile
// The row pass writes rows of kBtW = 64 floats: a whole bank row, so the four 16-lane groups of the column pass's
// ds_read_b128 (each 8 lanes of one tile row and 8 of the next, MI355X LDS banking) fall on 64 distinct banks.

inline int st_smooth_radius(double s) { return (int)(4.0 * s + 0.5); }

inline void st_smooth_taps(double s, int R, float* taps) {  // taps[k], k = 0 .. R (the kernel is symmetric)
  double k[kStMaxR + 1], sum = 0.0;
  for (int q = 0; q <= R; ++q) {
    k[q] = exp(-0.5 * (double)q * q / (s * s));
    sum += q ? 2.0 * k[q] : k[q];
  }
  for (int q = 0; q <= kStMaxR; ++q) taps[q] = q <= R ? (float)(k[q] / sum) : 0.f;
}

// one 1-D pass at N neighbouring centres p[0 .. N): taps[0] p[q] + sum_k taps[k] (p[q - k stride] + p[q + k stride])
template <int N>
DSX_ST_HD void st_tap_sum(const float* p, int stride, const float* taps, int R, float* out) {
  const StVec<float, N> c = *(const StVec<float, N>*)p;
#pragma unroll
  for (int q = 0; q < N; ++q) out[q] = taps[0] * c.v[q];
  for (int k = 1; k <= R; ++k) {
    const StVec<float, N> lo = *(const StVec<float, N>*)(p - k * stride);
    const StVec<float, N> hi = *(const StVec<float, N>*)(p + k * stride);
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = fmaf(taps[k], lo.v[q] + hi.v[q], out[q]);
  }
}

DSX_ST_HD float st_blend_px(int mode, float f, float b, float x, float w) {
  if (mode == kStSingle) return f;
  const float hi = mode == kStBg ? x : f, lo = mode == kStFg ? x : b;
  return hi * w + lo * (1.0f - w);
}

// flatfield_correction(r, flat, dark) of the float result, before the store's truncation
DSX_ST_HD float st_shade_px(float v, float flat, float dark) {
  v = v > dark ? v - dark : 0.f;
  v = v / flat;
  return fminf(fmaxf(v, 0.f), 65535.f);
}

template <typename TO>
DSX_ST_HD TO st_store_px(float v) {
  if (sizeof(TO) == 2) return (TO)(unsigned)fminf(fmaxf(v, 0.0f), 65535.0f);
  return (TO)v;
}

// Band loaders: where band `slot` of real plane b keeps pixel (i, j), which slot a band has, and band value from r.
struct StGenericBands {  // [P][Hp][Wp], band-major: the background (or only) band first, then the foreground
  int nb, Hp, Wp;
  DSX_ST_HD size_t at(int slot, int b, int i, int j) const {
    return ((size_t)slot * nb + b) * ((size_t)Hp * Wp) + (size_t)i * Wp + j;
  }
  DSX_ST_HD int fg_slot(int mode) const { return mode == kStBoth ? 1 : 0; }
  DSX_ST_HD int bg_slot(int) const { return 0; }
  static DSX_ST_HD float value(float r) { return expm1f(r); }
};
struct StMarchBands {  // virtual planes bands * b (foreground or only band) and bands * b + 1 (background), band + 2
  int bands, W;
  size_t px;
  DSX_ST_HD size_t at(int slot, int b, int i, int j) const {
    return ((size_t)bands * b + slot) * px + (size_t)i * W + j;
  }
  DSX_ST_HD int fg_slot(int) const { return 0; }
  DSX_ST_HD int bg_slot(int mode) const { return mode == kStBoth ? 1 : 0; }
  static DSX_ST_HD float value(float r) { return r - 2.0f; }
};

struct BlendArgs {
  const void* in;     // [nb][H][W]
  const float* r;     // the band planes, laid out as the loader says
  void* out;          // [nb][H][W]
  const float* t;     // [nb]
  const float* flat;  // [H][W], or nullptr: no dark / flat step
  const float* dark;  // [>= H][dark_w]
  int H, W, dark_w, mode, R;
  int vec;            // W, the band pitch and dark_w are multiples of 4 and every pointer is 16-byte aligned
  float inv_crossover;
  float taps[kStMaxR + 1];
};

// n <= 4 pixels from p into dst (the rest 0); vec: one 16- (float) or 8-byte (uint16) access
template <typename T>
__device__ __forceinline__ void st_load4(const T* p, bool vec, int n, float* dst) {
  if (vec) {
    const StVec<T, 4> v = *(const StVec<T, 4>*)p;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = (float)v.v[q];
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = q < n ? (float)p[q] : 0.f;
  }
}

// grid (ceil(W / 64), ceil(H / 16), planes); SMOOTH: a.R >= 1 and the weight goes through the two LDS passes
template <typename L, typename TI, typename TO, bool SMOOTH>
__global__ __launch_bounds__(256) void k_st_blendx(BlendArgs a, L ld) {
  constexpr int kRows = kBtH + 2 * kStMaxR;
  __shared__ float sw[SMOOTH ? kRows * kBtPitch0 : 1];                     // sigmoid of tile + halo
  __shared__ __attribute__((aligned(16))) float sh[SMOOTH ? kRows * kBtW : 4];  // after the row pass
  __shared__ __attribute__((aligned(16))) float sx[SMOOTH ? kBtH * kBtW : 4];   // x of the tile
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int b = blockIdx.z, i0 = blockIdx.y * kBtH, j0 = blockIdx.x * kBtW;
  const int i = i0 + ty, j = j0 + 4 * tx;
  const float tb = a.t[b];
  const TI* xin = (const TI*)a.in + (size_t)b * a.H * a.W;
  const int mode = a.mode;
  const bool vec = a.vec != 0;
  float w[4] = {0.f, 0.f, 0.f, 0.f}, x[4] = {0.f, 0.f, 0.f, 0.f};
  if (SMOOTH) {
    const int R = a.R, th = kBtH + 2 * R, tw = kBtW + 2 * R;
    for (int e = tid; e < th * tw; e += 256) {
      const int rr = e / tw, cc = e - rr * tw;
      int gi = i0 + rr - R, gj = j0 + cc - R;
      if ((unsigned)gi >= (unsigned)a.H) gi = st_refl(gi, a.H);
      if ((unsigned)gj >= (unsigned)a.W) gj = st_refl(gj, a.W);
      const float xv = pix(xin, (size_t)gi * a.W + gj);
      sw[rr * kBtPitch0 + cc] = st_weight(xv, tb, a.inv_crossover);
      if (rr >= R && rr < R + kBtH && cc >= R && cc < R + kBtW) sx[(rr - R) * kBtW + (cc - R)] = xv;
    }
    __syncthreads();
    for (int e = tid; e < th * kBtW; e += 256) {
      const int rr = e >> 6, cc = e & 63;
      st_tap_sum<1>(&sw[rr * kBtPitch0 + cc + R], 1, a.taps, R, &sh[rr * kBtW + cc]);
    }
    __syncthreads();
    st_tap_sum<4>(&sh[(ty + R) * kBtW + 4 * tx], kBtW, a.taps, R, w);
    const StVec<float, 4> xs = *(const StVec<float, 4>*)&sx[ty * kBtW + 4 * tx];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = xs.v[q];
  }
  if (i >= a.H || j >= a.W) return;
  const int n = min(4, a.W - j);
  const size_t o = (size_t)i * a.W + j;
  if (!SMOOTH && mode != kStSingle) {
    st_load4(xin + o, vec, n, x);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = st_weight(x[q], tb, a.inv_crossover);
  }
  float f[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
  if (mode != kStBg) st_load4(a.r + ld.at(ld.fg_slot(mode), b, i, j), vec, n, f);
  if (mode == kStBoth || mode == kStBg) st_load4(a.r + ld.at(ld.bg_slot(mode), b, i, j), vec, n, g);
  float fl[4] = {1.f, 1.f, 1.f, 1.f}, dk[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.flat != nullptr) {
    st_load4(a.flat + o, vec, n, fl);
    st_load4(a.dark + (size_t)i * a.dark_w + j, vec, n, dk);
  }
  StVec<TO, 4> ov;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float res = st_blend_px(mode, L::value(f[q]), L::value(g[q]), x[q], w[q]);
    if (a.flat != nullptr) res = st_shade_px(res, fl[q], dk[q]);
    ov.v[q] = st_store_px<TO>(res);
  }
  TO* dst = (TO*)a.out + (size_t)b * a.H * a.W + o;
  if (vec) {
    *(StVec<TO, 4>*)dst = ov;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < n) dst[q] = ov.v[q];
  }
}

// The blend of ONE plane on the host, from the functions above: x, f, b [H][W] float32 (f / b may be nullptr where the
// mode does not read them), band values as they are (no loader), out [H][W] float32 or uint16.
template <typename TO>
inline void st_blend_host(const float* x, const float* f, const float* b, int H, int W, float t, float inv_crossover,
                          int mode, double smoothing, const float* flat, const float* dark, int dark_w, TO* out) {
  const size_t px = (size_t)H * W;
  std::vector<float> w(px, 0.f);
  if (mode != kStSingle) {
    for (size_t k = 0; k < px; ++k) w[k] = st_weight(x[k], t, inv_crossover);
    const int R = smoothing > 0.0 ? st_smooth_radius(smoothing) : 0;
    if (R > 0) {
      float taps[kStMaxR + 1];
      st_smooth_taps(smoothing, R, taps);
      // each pass over a line folded out to R on both sides, as the kernel's LDS tile is
      std::vector<float> line((size_t)std::max(H, W) + 2 * R), tmp(px);
      for (int i = 0; i < H; ++i) {
        for (int c = -R; c < W + R; ++c) line[c + R] = w[(size_t)i * W + st_refl(c, W)];
        for (int c = 0; c < W; ++c) st_tap_sum<1>(&line[c + R], 1, taps, R, &tmp[(size_t)i * W + c]);
      }
      for (int c = 0; c < W; ++c) {
        for (int i = -R; i < H + R; ++i) line[i + R] = tmp[(size_t)st_refl(i, H) * W + c];
        for (int i = 0; i < H; ++i) st_tap_sum<1>(&line[i + R], 1, taps, R, &w[(size_t)i * W + c]);
      }
    }
  }
  for (int i = 0; i < H; ++i)
    for (int c = 0; c < W; ++c) {
      const size_t k = (size_t)i * W + c;
      float res = st_blend_px(mode, f ? f[k] : 0.f, b ? b[k] : 0.f, x[k], w[k]);
      if (flat != nullptr) res = st_shade_px(res, flat[k], dark[(size_t)i * dark_w + c]);
      out[k] = st_store_px<TO>(res);
    }
}

// ---- host side: geometry of a plan and the row-filter operators ---------------------------------------------------
constexpr int kStMaxLevels = 32;

struct StLevel {
  int h, w;          // cH_l shape
  int rh, rw;        // shape of the reconstruction of this level's approximation (from level l + 1; <= h + 1, w + 1)
  size_t a, ch, cv, cd, cf;  // region offsets (floats) in the workspace: approx, cH, cV, cD, filtered cH
  size_t mat[2];     // per band: offset (floats) of U [w][K] in the operator blob, V [K][w] follows
  int rank[2];       // K per band
};

struct StreaksPlan {
  int H = 0, W = 0, Hp = 0, Wp = 0, L = 0, F = 0, bands = 1, B = 0;
  int clip = 0;  // one band (bands == 1) of a clipped plane: kStFg max(x, t), kStBg min(x, t); 0: the plane itself
  float sigma[2] = {0.f, 0.f};  // band 0 (background / single), band 1 (foreground)
  float crossover = 10.f, threshold = 0.f;
  int otsu = 1;
  StLevel lv[kStMaxLevels];
  size_t y = 0, t0 = 0, t1 = 0;  // region offsets: padded log plane / level-0 reconstruction, two pass temporaries
  size_t ws_floats = 0, mat_floats = 0;
  Taps dec, rec;
};

inline int st_max_level(int n, int F) {  // pywt.dwt_max_level
  if (n < F - 1) return 0;
  int l = 0;
  for (long long q = n / (F - 1); q > 1; q >>= 1) ++l;
  return l;
}

// Low-rank form of the notch: x -> fftpack.irfft(fftpack.rfft(x) * g), g[q] = 1 - exp(-q^2 / (2 s^2)) on the PACKED
// index q (the reference's gaussian_filter), equals x + (x U) V with
//   U[k][q] = packed rfft basis: 1 (q = 0), cos(2 pi m k / n) (q = 2m - 1), -sin(2 pi m k / n) (q = 2m),
//             (-1)^k (q = n - 1, n even: the Nyquist term)
//   V[q][j] = -(1 - g[q]) * packed irfft basis: 1 / n, 2 cos(2 pi m j / n) / n, -2 sin(2 pi m j / n) / n, (-1)^j / n
// and only the first K packed indices carry 1 - g[q] = exp(-q^2 / (2 s^2)) >= 1e-9 relative (q < 6.44 s): beyond
// them the term is below float32 resolution of the row.  Returns K; U is [n][K], V is [K][n].
inline int st_notch_rank(int n, double s) { return std::min(n, (int)ceil(6.44 * s) + 1); }

inline void st_notch_factors(int n, double s, int K, float* U, float* V) {
  std::vector<double> cs((size_t)n), sn((size_t)n);
  for (int q = 0; q < n; ++q) {
    cs[q] = cos(2.0 * M_PI * q / n);
    sn[q] = sin(2.0 * M_PI * q / n);
  }
  for (int q = 0; q < K; ++q) {
    const double lowpass = exp(-((double)q * q) / (2.0 * s * s));  // 1 - g[q]
    const bool nyquist = (n & 1) == 0 && q == n - 1;
    const int m = (q + 1) / 2;
    for (int k = 0; k < n; ++k) {
      const size_t r = (size_t)(((long long)m * k) % n);
      double u, v;
      if (q == 0) { u = 1.0; v = 1.0 / n; }
      else if (nyquist) { u = (k & 1) ? -1.0 : 1.0; v = u / n; }
      else if (q & 1) { u = cs[r]; v = 2.0 * cs[r] / n; }
      else { u = -sn[r]; v = -2.0 * sn[r] / n; }
      U[(size_t)k * K + q] = (float)u;
      V[(size_t)q * n + k] = (float)(-lowpass * v);
    }
  }
}

// Geometry of a plan for P = bands * B virtual planes; returns false when a level count is out of range
inline bool st_build_plan(StreaksPlan& p, int level) {
  p.Hp = p.H + (p.H & 1);
  p.Wp = p.W + (p.W & 1);
  p.L = level > 0 ? level : st_max_level(std::min(p.Hp, p.Wp), p.F);
  if (p.L >= kStMaxLevels) return false;
  const size_t P = (size_t)p.bands * p.B;
  size_t off = 0;
  auto region = [&](size_t floats) { const size_t o = off; off += floats * P; return o; };
  p.y = region((size_t)p.Hp * p.Wp);
  int h = p.Hp, w = p.Wp;
  size_t tmp = 0, mat = 0;
  for (int l = 0; l < p.L; ++l) {
    StLevel& v = p.lv[l];
    tmp = std::max(tmp, (size_t)((h + p.F - 1) / 2) * (w + 1));
    v.h = (h + p.F - 1) / 2;
    v.w = (w + p.F - 1) / 2;
    v.a = region((size_t)(v.h + 1) * (v.w + 1));
    v.ch = region((size_t)v.h * v.w);
    v.cv = region((size_t)v.h * v.w);
    v.cd = region((size_t)v.h * v.w);
    v.cf = region((size_t)v.h * v.w);
    for (int b = 0; b < p.bands; ++b) {
      v.rank[b] = st_notch_rank(v.w, (double)v.h * p.sigma[b] / p.Hp);
      v.mat[b] = mat;
      mat += 2 * (size_t)v.w * v.rank[b];
    }
    h = v.h;
    w = v.w;
  }
  for (int l = 0; l < p.L; ++l) {  // what the inverse pass of level l + 1 rebuilds in place of approx l
    if (l + 1 < p.L) {
      p.lv[l].rh = 2 * p.lv[l + 1].h - p.F + 2;
      p.lv[l].rw = 2 * p.lv[l + 1].w - p.F + 2;
    } else {
      p.lv[l].rh = p.lv[l].h;
      p.lv[l].rw = p.lv[l].w;
    }
    if (p.lv[l].rh > p.lv[l].h + 1 || p.lv[l].rw > p.lv[l].w + 1 || p.lv[l].rh < p.lv[l].h || p.lv[l].rw < p.lv[l].w)
      return false;
  }
  p.t0 = region(tmp);
  p.t1 = region(tmp);
  p.ws_floats = off;
  p.mat_floats = mat;
  return true;
}

}  // namespace st
}  // namespace dsx

#endif  // DSX_STREAKS_H
