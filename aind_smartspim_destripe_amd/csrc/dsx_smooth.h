// dsx_smooth.h -- the finish of a retrospective flat on the device (gfx950), and its host build: masked median fill,
// separable float64 Gaussian, strided mean, normalisation.
//
// aind_smartspim_destripe_amd/flatfield_estimation.py makes a flat from the per-pixel rank planes of dsx_stackrank.h by
// filling unseen pixels, smoothing with scipy's Gaussian restated in NumPy and dividing by the mean.  The rank planes lie
// in device memory; this header finishes the flat there.  The contract ("native finish", include/dsx.h) fixes the order
// of every float64 operation, so the kernels and the plain C++ below agree bit for bit:
//
//   fold  m(j): j' = j mod 2n (non-negative); m = j' < n ? j' : 2n - 1 - j'          (np.pad(mode="symmetric"))
//   tap   acc = t_0 * a[i];  k = 1 .. r:  acc = fma(t_k, a[m(i - k)] + a[m(i + k)], acc)   axis 0 first, then axis 1
//   mean  p_j = sum of S[i], i = j (mod 4096), increasing i, from 0.0;  mean = (p_0 + p_1 + ... left to right) / N
//   flat  float32(q < floor ? floor : q), q = S / mean (IEEE division);  dark = float32(S_dark)
//   fill  the median of the seen pixels of the crop from a 65 536-bin count: (v_(M-1)/2 + v_M/2) / 2, exact
// Every multiply-add is spelled __builtin_fma; no expression of the form a * b + c is left for a compiler to contract.
//
// Kernels (all launches of 256 threads, lanes along x, so global accesses are coalesced):
//   k_sm_hist    masked count of the H x W crop.  A block counts the values below 16 384 in LDS (64 KiB, as k_volhist_u16)
//                and the others in the global bins; a wave whose counted lanes hold one value adds once.
//   k_sm_median  one block: prefix sums over the bins, leaves fill and the seen count M in device memory.
//   k_sm_fill    convert, crop and fill to a dense float64 [H][W].
//   k_sm_col     axis 0.  A block owns 32 columns x 32 output rows; LDS holds the 32 + 2r window rows [row][32], folded
//                by m at load time.  A thread is column t % 32 and the rows t / 32 + 8u, u < 4: four accumulators, and
//                the two halves of a wave read two adjacent 256-byte rows -- no bank conflict with ds_read_b64.
//   k_sm_row     axis 1.  A block owns 64 outputs along x of 16 rows; LDS holds [16][64 + 2 r'] with r' = r rounded up
//                to even, so that the window starts on an even column.  A thread is output t % 64 of the rows
//                t / 64 + 4u, u < 4.
//                Both passes load with 16 bytes per lane where W is even and the base is 16-byte aligned (pairs that the
//                fold breaks are loaded singly), and with 8 bytes per lane otherwise.  Taps arrive as a kernel argument:
//                t_k is a scalar load, the FMA takes it from SGPRs.  Two LDS reads per FMA, each a ds_read_b64
//                (sm_read): the passes are LDS-bound.
//                LDS: (32 + 2r) * 256 bytes and 16 * (64 + 2r') * 8 bytes: 72 KiB and 40 KiB at r = 128 (two and three
//                blocks per CU), 136 KiB and 72 KiB at r = 256.
//   k_sm_partial 4096 threads, thread j adds S[j], S[j + 4096], ... in order (sixteen loads in flight).
//   k_sm_mean    one block: the 4096 partial sums, left to right, divided by N.
//   k_sm_norm / k_sm_f32   the flat and the dark as float32.
// No atomics outside k_sm_hist, no scratch.
#ifndef DSX_SMOOTH_H
#define DSX_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define DSX_SM_HD __host__ __device__
#else
#define DSX_SM_HD
#endif

// the host loops below once more for CPUs with FMA and AVX2 (the same operations, so the same bits)
#if defined(__x86_64__) && defined(__linux__) && !defined(__HIP_DEVICE_COMPILE__) && !defined(DSX_SM_NO_CLONES)
#define DSX_SM_CLONES __attribute__((target_clones("default", "arch=haswell")))
#else
#define DSX_SM_CLONES
#endif

namespace dsx {
namespace sm {

constexpr int kSmThreads = 256;
constexpr int kSmMaxRadius = 256;   // sigma <= 64
constexpr int kSmColTx = 32;        // k_sm_col: columns and output rows of a tile
constexpr int kSmColTy = 32;
constexpr int kSmRowTx = 64;        // k_sm_row: outputs along x and rows of a tile
constexpr int kSmRowTy = 16;
constexpr int kSmMeanLanes = 4096;  // L of the mean
constexpr int kSmBins = 65536;      // one bin per uint16 value
constexpr int kSmWin = 16384;       // values k_sm_hist counts in LDS
constexpr long long kSmMaxElems = ((long long)1 << 31) - 1;

struct Taps {
  double t[kSmMaxRadius + 1];  // centre and right half
};

// what k_sm_median leaves and k_sm_mean adds
struct Scalars {
  double fill;
  double mean;
  unsigned long long seen;
};

// m(j) of the contract for an axis of length n
DSX_SM_HD inline long long fold(long long j, long long n) {
  const long long p = 2 * n;
  long long q = j % p;
  if (q < 0) q += p;
  return q < n ? q : p - 1 - q;
}

// one tap of the contract
DSX_SM_HD inline double tap(double tk, double below, double above, double acc) { return __builtin_fma(tk, below + above, acc); }

// one flat value of the contract (a NaN quotient stays NaN, as np.maximum keeps it)
DSX_SM_HD inline float flat_value(double s, double mean, double floor) {
  const double q = s / mean;
  return (float)(q < floor ? floor : q);
}

// The argument rules of the two passes; nullptr when the call may run.
inline const char* check_smooth(const void* in, long long H, long long W, const double* taps, int radius, const void* tmp,
                                const void* out) {
  if (radius < 0 || radius > kSmMaxRadius) return "gauss_smooth: 0 <= radius <= 256";
  if (H < 1 || W < 1 || H > kSmMaxElems || W > kSmMaxElems || H * W > kSmMaxElems) return "gauss_smooth: 1 <= H, W and H * W < 2^31";
  if (!in || !taps || !tmp || !out) return "gauss_smooth: NULL pointer";
  if (tmp == in || tmp == out) return "gauss_smooth: tmp must be a buffer of its own";
  if (((uintptr_t)in | (uintptr_t)tmp | (uintptr_t)out) & 7) return "gauss_smooth: float64 planes must be 8-byte aligned";
  return nullptr;
}

// The argument rules of the finish; nullptr when the call may run.
inline const char* check_finish(const void* rank, const void* valid, long long Hs, long long Ws, long long H, long long W,
                                int n_q, const double* taps, int radius, double floor, const void* flat, const void* dark) {
  if (radius < 0 || radius > kSmMaxRadius) return "flat_finish: 0 <= radius <= 256";
  if (n_q < 1 || n_q > 2) return "flat_finish: n_q is 1 (flat) or 2 (flat, dark)";
  if (H < 1 || W < 1 || H > kSmMaxElems || W > kSmMaxElems || H * W > kSmMaxElems) return "flat_finish: 1 <= H, W and H * W < 2^31";
  if (Hs < H || Ws < W || Hs > kSmMaxElems || Ws > kSmMaxElems || Hs * Ws > kSmMaxElems)
    return "flat_finish: the image is the top-left crop of the stored planes, Hs * Ws < 2^31";
  if (!(floor > 0.0) || !(floor < 1e300)) return "flat_finish: floor must be positive and finite";
  if (!rank || !valid || !taps || !flat || (n_q == 2 && !dark)) return "flat_finish: NULL pointer";
  if (((uintptr_t)rank | (uintptr_t)valid) & 1) return "flat_finish: uint16 planes must be 2-byte aligned";
  if (((uintptr_t)flat | (uintptr_t)dark) & 3) return "flat_finish: float32 results must be 4-byte aligned";
  return nullptr;
}

// What the launches of the two passes over an H x W plane with radius r look like (arguments inside the limits).
struct Geometry {
  int col_tx, col_ty;        // k_sm_col: columns and output rows of a tile
  int row_tx, row_ty;        // k_sm_row: outputs along x and rows of a tile
  int col_rows;              // window rows of a column tile: col_ty + 2 r
  int row_pad, row_pitch;    // r rounded up to even; window columns of a row tile: row_tx + 2 row_pad
  size_t col_lds, row_lds;   // dynamic LDS of the two launches
  unsigned col_bx, col_by;   // tiles along x and y; the launch is 1-D, col_bx * col_by blocks
  unsigned row_bx, row_by;
};
inline Geometry geometry(long long H, long long W, int r) {
  Geometry g;
  g.col_tx = kSmColTx, g.col_ty = kSmColTy, g.row_tx = kSmRowTx, g.row_ty = kSmRowTy;
  g.col_rows = g.col_ty + 2 * r;
  g.row_pad = r + (r & 1);
  g.row_pitch = g.row_tx + 2 * g.row_pad;
  g.col_lds = (size_t)g.col_rows * (size_t)g.col_tx * sizeof(double);
  g.row_lds = (size_t)g.row_ty * (size_t)g.row_pitch * sizeof(double);
  g.col_bx = (unsigned)((W + g.col_tx - 1) / g.col_tx), g.col_by = (unsigned)((H + g.col_ty - 1) / g.col_ty);
  g.row_bx = (unsigned)((W + g.row_tx - 1) / g.row_tx), g.row_by = (unsigned)((H + g.row_ty - 1) / g.row_ty);
  return g;
}
constexpr size_t kSmMaxLds = (size_t)(kSmColTy + 2 * kSmMaxRadius) * kSmColTx * sizeof(double);  // 136 KiB

// Layout of the work buffer of the finish: bins, scalars, partial sums, two float64 planes.
struct Work {
  size_t hist, scal, part, a, tmp, bytes;
};
inline Work work_layout(long long H, long long W) {
  Work w;
  w.hist = 0;
  w.scal = w.hist + (size_t)kSmBins * sizeof(unsigned);
  w.part = w.scal + 256;
  w.a = w.part + (size_t)kSmMeanLanes * sizeof(double);
  w.tmp = w.a + (((size_t)H * (size_t)W * sizeof(double) + 255) & ~(size_t)255);
  w.bytes = w.tmp + (size_t)H * (size_t)W * sizeof(double);
  return w;
}

// fill and M from the bins: M = all counts; fill = (v_(M-1)/2 + v_M/2) / 2 over the sorted seen values; 0 when M == 0
inline double median_of_bins(const unsigned* hist, unsigned long long* seen) {
  unsigned long long M = 0;
  for (int v = 0; v < kSmBins; ++v) M += hist[v];
  *seen = M;
  if (!M) return 0.0;
  const unsigned long long k1 = (M - 1) / 2, k2 = M / 2;
  unsigned long long cum = 0;
  unsigned v1 = 0, v2 = 0;
  for (int v = 0; v < kSmBins; ++v) {
    const unsigned long long c = hist[v];
    if (k1 >= cum && k1 < cum + c) v1 = (unsigned)v;
    if (k2 >= cum && k2 < cum + c) v2 = (unsigned)v;
    cum += c;
  }
  return 0.5 * (double)(v1 + v2);
}

DSX_SM_CLONES static void sm_scale(double* acc, const double* a, double t0, size_t n) {
  for (size_t x = 0; x < n; ++x) acc[x] = t0 * a[x];
}
DSX_SM_CLONES static void sm_taps(double* acc, const double* below, const double* above, double tk, size_t n) {
  for (size_t x = 0; x < n; ++x) acc[x] = tap(tk, below[x], above[x], acc[x]);
}

// The two passes on the host: in -> tmp along axis 0, tmp -> out along axis 1.  out may be in.
inline void smooth_host(const double* in, long long H, long long W, const double* t, int r, double* tmp, double* out) {
  for (long long i = 0; i < H; ++i) {
    double* acc = tmp + i * W;
    sm_scale(acc, in + i * W, t[0], (size_t)W);
    for (int k = 1; k <= r; ++k) sm_taps(acc, in + fold(i - k, H) * W, in + fold(i + k, H) * W, t[k], (size_t)W);
  }
  std::vector<double> line((size_t)W + 2 * (size_t)r);
  for (long long i = 0; i < H; ++i) {
    const double* row = tmp + i * W;
    for (long long j = 0; j < W + 2 * r; ++j) line[(size_t)j] = row[fold(j - r, W)];
    double* acc = out + i * W;
    const double* c = line.data() + r;
    sm_scale(acc, c, t[0], (size_t)W);
    for (int k = 1; k <= r; ++k) sm_taps(acc, c - k, c + k, t[k], (size_t)W);
  }
}

// mean of the contract over N values
inline double mean_host(const double* S, long long N) {
  std::vector<double> p(kSmMeanLanes, 0.0);
  for (long long i0 = 0; i0 < N; i0 += kSmMeanLanes) {
    const long long m = N - i0 < kSmMeanLanes ? N - i0 : kSmMeanLanes;
    for (long long j = 0; j < m; ++j) p[(size_t)j] = p[(size_t)j] + S[i0 + j];
  }
  double s = p[0];
  for (int j = 1; j < kSmMeanLanes; ++j) s = s + p[(size_t)j];
  return s / (double)N;
}

// The finish on the host (arguments as check_finish passed them).  Returns false, with nothing written, when no pixel
// of the crop is seen.
inline bool flat_finish_host(const uint16_t* rank, const uint16_t* valid, long long Hs, long long Ws, long long H, long long W,
                             int n_q, const double* t, int r, double floor, float* flat, float* dark) {
  const long long N = H * W;
  std::vector<unsigned> hist(kSmBins);
  std::vector<double> a((size_t)N), tmp((size_t)N);
  for (int q = 0; q < n_q; ++q) {
    const uint16_t* R = rank + (size_t)q * (size_t)Hs * (size_t)Ws;
    hist.assign(kSmBins, 0u);
    for (long long y = 0; y < H; ++y)
      for (long long x = 0; x < W; ++x)
        if (valid[y * Ws + x]) ++hist[R[y * Ws + x]];
    unsigned long long seen = 0;
    const double fill = median_of_bins(hist.data(), &seen);
    if (!seen) return false;
    for (long long y = 0; y < H; ++y)
      for (long long x = 0; x < W; ++x) a[(size_t)(y * W + x)] = valid[y * Ws + x] ? (double)R[y * Ws + x] : fill;
    smooth_host(a.data(), H, W, t, r, tmp.data(), a.data());
    if (q == 0) {
      const double mean = mean_host(a.data(), N);
      for (long long i = 0; i < N; ++i) flat[i] = flat_value(a[(size_t)i], mean, floor);
    } else {
      for (long long i = 0; i < N; ++i) dark[i] = (float)a[(size_t)i];
    }
  }
  return true;
}

}  // namespace sm
}  // namespace dsx

#if defined(__HIP__)

namespace dsx {
namespace sm {

typedef double sm_f64x2 __attribute__((ext_vector_type(2)));

// One 8-byte LDS read of the tap loops.  A relaxed wave-scope atomic load is an ordinary load that the compiler does not
// pair with its neighbour: plain loads of the unrolled loop become ds_read2_b64, which moves half the bytes per LDS
// cycle of ds_read_b64, and the passes are LDS-bound.
__device__ __forceinline__ double sm_read(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// grid: any number of blocks (the launch takes two per CU, fewer for small planes).  hist: kSmBins zeroed bins.
__global__ __launch_bounds__(kSmThreads) void k_sm_hist(const uint16_t* __restrict__ R, const uint16_t* __restrict__ valid,
                                                        int Ws, int W, int N, unsigned* __restrict__ hist) {
  __shared__ unsigned win[kSmWin];
  for (int k = threadIdx.x; k < kSmWin; k += kSmThreads) win[k] = 0u;
  __syncthreads();
  const long long stride = (long long)gridDim.x * kSmThreads;
  // (the loop bound is the same for every thread of a block, so the ballots below see whole waves)
  for (long long base = (long long)blockIdx.x * kSmThreads; base < (long long)N; base += stride) {
    const long long i = base + threadIdx.x;
    bool counted = false;
    unsigned v = 0u;
    if (i < (long long)N) {
      const unsigned y = (unsigned)i / (unsigned)W, x = (unsigned)i - y * (unsigned)W;  // i < 2^31
      const size_t at = (size_t)y * (size_t)Ws + x;
      counted = valid[at] != 0;
      v = R[at];
    }
    const unsigned long long act = __ballot(counted);
    if (act == 0ull) continue;
    const unsigned first = (unsigned)__shfl((int)v, __ffsll((long long)act) - 1);
    const unsigned long long uni = __ballot(counted && v == first);
    unsigned c = counted ? 1u : 0u;
    if (uni == act) {  // the counted lanes hold one value: its first lane adds for all
      c = (threadIdx.x & 63) == __ffsll((long long)act) - 1 ? (unsigned)__popcll(act) : 0u;
    }
    if (c) {
      if (v < (unsigned)kSmWin) atomicAdd(&win[v], c);
      else atomicAdd(&hist[v], c);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kSmWin; k += kSmThreads) {
    const unsigned c = win[k];
    if (c) atomicAdd(&hist[k], c);
  }
}

// one block of kSmThreads threads: thread t owns the bins 256 t .. 256 t + 255
__global__ __launch_bounds__(kSmThreads) void k_sm_median(const unsigned* __restrict__ hist, Scalars* __restrict__ scal) {
  __shared__ unsigned long long before[kSmThreads + 1];
  __shared__ unsigned found[2];
  constexpr int kOwn = kSmBins / kSmThreads;
  const int t = threadIdx.x;
  unsigned long long s = 0;
  for (int b = 0; b < kOwn; ++b) s += hist[t * kOwn + b];
  before[t + 1] = s;
  if (t < 2) found[t] = 0u;
  __syncthreads();
  if (t == 0) {
    before[0] = 0;
    for (int k = 1; k <= kSmThreads; ++k) before[k] += before[k - 1];
  }
  __syncthreads();
  const unsigned long long M = before[kSmThreads];
  if (M) {
    const unsigned long long k1 = (M - 1) / 2, k2 = M / 2;
    unsigned long long cum = before[t];
    if (k1 < before[t + 1] && k2 >= cum) {  // (k1 <= k2: one of them may lie in this thread's bins)
      for (int b = 0; b < kOwn; ++b) {
        const unsigned long long c = hist[t * kOwn + b];
        if (k1 >= cum && k1 < cum + c) found[0] = (unsigned)(t * kOwn + b);
        if (k2 >= cum && k2 < cum + c) found[1] = (unsigned)(t * kOwn + b);
        cum += c;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    scal->fill = M ? 0.5 * (double)(found[0] + found[1]) : 0.0;
    scal->seen = M;
  }
}

// grid: blocks of kSmThreads threads that cover N = H * W
__global__ __launch_bounds__(kSmThreads) void k_sm_fill(const uint16_t* __restrict__ R, const uint16_t* __restrict__ valid,
                                                        int Ws, int W, int N, const Scalars* __restrict__ scal,
                                                        double* __restrict__ a) {
  const long long i = (long long)blockIdx.x * kSmThreads + threadIdx.x;
  if (i >= (long long)N) return;
  const unsigned y = (unsigned)i / (unsigned)W, x = (unsigned)i - y * (unsigned)W;  // i < 2^31
  const size_t at = (size_t)y * (size_t)Ws + x;
  a[i] = valid[at] ? (double)R[at] : scal->fill;
}

// grid: geometry(H, W, r).col_bx * col_by blocks; dynamic LDS: col_lds.  vec: W is even and in is 16-byte aligned.
__global__ __launch_bounds__(kSmThreads) void k_sm_col(const double* __restrict__ in, double* __restrict__ out, int H, int W,
                                                       int r, unsigned bx_n, Taps taps, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sm_lds[];
  const int t = threadIdx.x;
  const long long x0 = (long long)(blockIdx.x % bx_n) * kSmColTx, y0 = (long long)(blockIdx.x / bx_n) * kSmColTy;
  const int rows = kSmColTy + 2 * r;
  if (vec) {
    const int pc = (t & 15) * 2;
    if (x0 + pc < W)
      for (int j = t >> 4; j < rows; j += kSmThreads / 16) {
        const long long gy = fold(y0 - r + j, H);
        *reinterpret_cast<sm_f64x2*>(sm_lds + j * kSmColTx + pc) =
            *reinterpret_cast<const sm_f64x2*>(in + (size_t)gy * (size_t)W + (size_t)(x0 + pc));
      }
  } else {
    const int c = t & 31;
    if (x0 + c < W)
      for (int j = t >> 5; j < rows; j += kSmThreads / 32) {
        const long long gy = fold(y0 - r + j, H);
        sm_lds[j * kSmColTx + c] = in[(size_t)gy * (size_t)W + (size_t)(x0 + c)];
      }
  }
  __syncthreads();

  // column c of the output rows i0 + 8 u: window row i + r is the centre.  Columns past W hold nothing that is stored.
  const int c = t & 31, i0 = t >> 5;
  const double* mid = sm_lds + (i0 + r) * kSmColTx + c;
  double acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = taps.t[0] * mid[u * 8 * kSmColTx];
  for (int k = 1; k <= r; ++k) {
    const double tk = taps.t[k];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc[u] = tap(tk, sm_read(mid + (u * 8 - k) * kSmColTx), sm_read(mid + (u * 8 + k) * kSmColTx), acc[u]);
  }
  if (x0 + c < W) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long y = y0 + i0 + u * 8;
      if (y < H) out[(size_t)y * (size_t)W + (size_t)(x0 + c)] = acc[u];
    }
  }
}

// grid: geometry(H, W, r).row_bx * row_by blocks; dynamic LDS: row_lds.  vec: W is even and in is 16-byte aligned.
__global__ __launch_bounds__(kSmThreads) void k_sm_row(const double* __restrict__ in, double* __restrict__ out, int H, int W,
                                                       int r, unsigned bx_n, Taps taps, int vec) {
  extern __shared__ __attribute__((aligned(16))) double sm_lds[];
  const int t = threadIdx.x;
  const long long x0 = (long long)(blockIdx.x % bx_n) * kSmRowTx, y0 = (long long)(blockIdx.x / bx_n) * kSmRowTy;
  const int pad = r + (r & 1), pitch = kSmRowTx + 2 * pad;
  if (vec) {
    const int pairs = pitch / 2;
    for (int idx = t; idx < kSmRowTy * pairs; idx += kSmThreads) {
      const int row = idx / pairs, j = 2 * (idx - row * pairs);
      if (y0 + row >= H) break;  // (rows grow with idx)
      const double* src = in + (size_t)(y0 + row) * (size_t)W;
      const long long gx = x0 - pad + j;
      sm_f64x2 v;
      if (gx >= 0 && gx + 1 < W) {
        v = *reinterpret_cast<const sm_f64x2*>(src + gx);
      } else {
        v.x = src[fold(gx, W)];
        v.y = src[fold(gx + 1, W)];
      }
      *reinterpret_cast<sm_f64x2*>(sm_lds + row * pitch + j) = v;
    }
  } else {
    for (int idx = t; idx < kSmRowTy * pitch; idx += kSmThreads) {
      const int row = idx / pitch, j = idx - row * pitch;
      if (y0 + row >= H) break;
      sm_lds[row * pitch + j] = in[(size_t)(y0 + row) * (size_t)W + (size_t)fold(x0 - pad + j, W)];
    }
  }
  __syncthreads();

  // output c of the rows i0 + 4 u: window column pad + c is the centre.  Rows past H hold nothing that is stored.
  const int c = t & 63, i0 = t >> 6;
  const double* mid = sm_lds + i0 * pitch + pad + c;
  const int step = 4 * pitch;
  double acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = taps.t[0] * mid[u * step];
  for (int k = 1; k <= r; ++k) {
    const double tk = taps.t[k];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = tap(tk, sm_read(mid + u * step - k), sm_read(mid + u * step + k), acc[u]);
  }
  if (x0 + c < W) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long y = y0 + i0 + u * 4;
      if (y < H) out[(size_t)y * (size_t)W + (size_t)(x0 + c)] = acc[u];
    }
  }
}

// grid: kSmMeanLanes / kSmThreads blocks.  part[j] = S[j] + S[j + 4096] + ... in this order, from 0.0.
__global__ __launch_bounds__(kSmThreads) void k_sm_partial(const double* __restrict__ S, int N, double* __restrict__ part) {
  constexpr int kFlight = 16;
  const long long j = (long long)blockIdx.x * kSmThreads + threadIdx.x;
  double acc = 0.0;
  for (long long i = j; i < (long long)N; i += (long long)kFlight * kSmMeanLanes) {
    double v[kFlight];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const long long at = i + (long long)u * kSmMeanLanes;
      v[u] = at < (long long)N ? S[at] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kFlight; ++u)
      if (i + (long long)u * kSmMeanLanes < (long long)N) acc = acc + v[u];
  }
  part[j] = acc;
}

// one block: mean = (part[0] + part[1] + ... left to right) / N
__global__ __launch_bounds__(kSmThreads) void k_sm_mean(const double* __restrict__ part, int N, Scalars* __restrict__ scal) {
  __shared__ double p[kSmMeanLanes];
  for (int k = threadIdx.x; k < kSmMeanLanes; k += kSmThreads) p[k] = part[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = p[0];
    for (int k = 1; k < kSmMeanLanes; ++k) s = s + p[k];
    scal->mean = s / (double)N;
  }
}

// grid: blocks of kSmThreads threads that cover N
__global__ __launch_bounds__(kSmThreads) void k_sm_norm(const double* __restrict__ S, int N, const Scalars* __restrict__ scal,
                                                        double floor, float* __restrict__ flat) {
  const long long i = (long long)blockIdx.x * kSmThreads + threadIdx.x;
  if (i < (long long)N) flat[i] = flat_value(S[i], scal->mean, floor);
}

__global__ __launch_bounds__(kSmThreads) void k_sm_f32(const double* __restrict__ S, int N, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kSmThreads + threadIdx.x;
  if (i < (long long)N) out[i] = (float)S[i];
}

}  // namespace sm
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_SMOOTH_H */
