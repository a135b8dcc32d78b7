// dsx_project.h -- orthogonal maximum / sum projections of a uint16 volume that arrives in z blocks (gfx950), and the
// host build.
//
// A store pass leaves nothing a person can look at.  While a block's input and filtered planes lie dense in device
// memory as uint16 [Z, H, W], one more read of them gives the three maximum-intensity projections and the three sum
// projections; the row sums before and after the filter are the stripe signature and what became of it.
//
// For v[Z, H, W] and the rows z_off .. z_off + Z - 1 of the [., W] / [., H] arrays:
//     max_z[h, w] (uint16), sum_z[h, w] (uint64) : over z; overwritten when `first`, combined with what is there otherwise
//     max_y[z_off + z, w] (uint16), sum_y (uint32) : over h
//     max_x[z_off + z, h] (uint16), sum_x (uint32) : over w
// H, W <= 65 536: a uint32 sum of 65 536 values of 65 535 cannot overflow; Z <= 65 536 per call for the same reason (the
// z sums of one call are carried in 32 bits).  All integers: exact, whatever the order of the blocks.
//
//   k_project_u16 : the planes are read ONCE for all six outputs.  grid (strips, tiles): a block of 8 waves owns a tile
//       of 32 rows x 512 columns and marches over the planes; a wave owns 4 rows, a lane 8 columns of each (one 16-byte
//       load per row when W % 8 == 0 and the base is 16-byte aligned; eight 2-byte loads, lane-interleaved, otherwise:
//       the rule of k_pyramid_step).  The next plane's loads are issued before the current plane is reduced, and the
//       block barrier orders LDS traffic only, so they stay in flight across it.
//         z : 32 sums (uint32) and 16 packed maxima per lane stay in registers across the plane loop and are written
//             (or combined) once at the end.
//         x : a lane adds its 8 columns, the wave reduces its 4 rows across lanes in one butterfly and stores the strip's partial
//             [Z][strips][H].
//         y : a lane adds its 4 rows per column, the 8 waves meet in LDS (one barrier per plane, two buffers), 512
//             threads add the 8 waves' values of one column each and store the tile's partial [Z][tiles][W].
//       No atomics: an atomic per voxel per reduction would bound the kernel at the atomic rate, and even the few
//       per-strip x partials would arrive one lane per row, the slow shape.  Plain stores instead: the partials are
//       Z (tiles W + strips H) x 6 bytes, 10 % of the bytes read for a 1600 x 2000 plane, written once and read once.
//       Registers: 144 VGPRs, no scratch -- one block of 8 waves per CU with two planes of loads in flight per wave,
//       the same bytes in flight as two blocks with one plane each would have, and twice as many when the grid has
//       fewer blocks than the chip has CUs (a 1600 x 2000 plane has 200).
//   k_project_fold : one thread per element of the four [Z, .] rows adds / maximises its partials.
//
//   project_host : the same values on the host (dsx_project_u16_ref), plain C++.
#ifndef DSX_PROJECT_H
#define DSX_PROJECT_H

#include <stddef.h>
#include <stdint.h>

namespace dsx {
namespace pj {

constexpr int kPjMaxExtent = 65536;  // H, W, and Z of one call
constexpr int kPjThreads = 512;      // 8 waves
constexpr int kPjWaves = kPjThreads / 64;
constexpr int kPjRows = 4;                         // rows of a wave
constexpr int kPjTileRows = kPjWaves * kPjRows;    // rows of a block
constexpr int kPjCols = 8;                         // columns of a lane
constexpr int kPjStrip = 64 * kPjCols;             // columns of a block
constexpr int kPjPitch = 68;  // LDS row pitch in dwords: 64 lanes + 4, so that the column-major readers spread over the banks

struct Outputs {
  uint16_t* max_z; uint64_t* sum_z;  // [H, W]
  uint16_t* max_y; uint32_t* sum_y;  // [., W]
  uint16_t* max_x; uint32_t* sum_x;  // [., H]
};

inline int tiles(int H) { return (H + kPjTileRows - 1) / kPjTileRows; }
inline int strips(int W) { return (W + kPjStrip - 1) / kPjStrip; }

// d_work: uint32 y partials [Z][tiles][W], uint32 x partials [Z][strips][H], then the uint16 maxima in the same order
inline size_t partial_elems(int Z, int H, int W) {
  return (size_t)Z * ((size_t)tiles(H) * W + (size_t)strips(W) * H);
}
inline size_t work_bytes(int Z, int H, int W) { return (partial_elems(Z, H, W) * 6 + 15) / 16 * 16; }

// v: Z dense planes (2-byte aligned).  Rows z_off .. z_off + Z - 1 of the y / x arrays are written; the z arrays are
// overwritten when `first`, combined otherwise.
inline void project_host(const uint16_t* v, int Z, int H, int W, const Outputs& o, int z_off, bool first) {
  const size_t plane = (size_t)H * W;
  if (first)
    for (size_t i = 0; i < plane; ++i) { o.max_z[i] = 0; o.sum_z[i] = 0; }
  for (int z = 0; z < Z; ++z) {
    uint16_t* my = o.max_y + (size_t)(z_off + z) * W;
    uint32_t* sy = o.sum_y + (size_t)(z_off + z) * W;
    uint16_t* mx = o.max_x + (size_t)(z_off + z) * H;
    uint32_t* sx = o.sum_x + (size_t)(z_off + z) * H;
    for (int w = 0; w < W; ++w) { my[w] = 0; sy[w] = 0; }
    for (int h = 0; h < H; ++h) {
      const uint16_t* row = v + (size_t)z * plane + (size_t)h * W;
      uint16_t* mz = o.max_z + (size_t)h * W;
      uint64_t* sz = o.sum_z + (size_t)h * W;
      uint16_t m = 0;
      uint32_t s = 0;
      for (int w = 0; w < W; ++w) {
        const uint16_t x = row[w];
        if (x > m) m = x;
        s += x;
        if (x > my[w]) my[w] = x;
        sy[w] += x;
        if (x > mz[w]) mz[w] = x;
        sz[w] += x;
      }
      mx[h] = m;
      sx[h] = s;
    }
  }
}

}  // namespace pj
}  // namespace dsx

#if defined(__HIP__)
#include <hip/hip_runtime.h>

namespace dsx {
namespace pj {

typedef unsigned int pj_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short pj_u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long pj_u64x2 __attribute__((ext_vector_type(2)));

// two uint16 maxima per dword (v_pk_max_u16)
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(pj_u16x2, a),
                                                                __builtin_bit_cast(pj_u16x2, b)));
}

// A block barrier that orders LDS traffic only: global loads issued in front of it stay in flight across it (a
// __syncthreads would wait for them).  Nothing global is handed from thread to thread inside the kernel.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct Partials {
  unsigned* ysum; unsigned* xsum;  // [Z][tiles][W], [Z][strips][H]
  uint16_t* ymax; uint16_t* xmax;
};

__host__ __device__ inline Partials partials(void* work, int Z, int H, int W) {
  Partials p;
  p.ysum = (unsigned*)work;
  p.xsum = p.ysum + (size_t)Z * tiles(H) * W;
  p.ymax = (uint16_t*)(p.xsum + (size_t)Z * strips(W) * H);
  p.xmax = p.ymax + (size_t)Z * tiles(H) * W;
  return p;
}

// The 8 voxels of a lane in row `row` of one plane as four dwords (column j in half j & 1 of dword j >> 1); zeros --
// the identity of both reducers -- outside the plane.
template <bool VEC>
__device__ __forceinline__ void load_row(const uint16_t* __restrict__ plane, int row, int H, int W, int c0, int lane,
                                         unsigned d[4]) {
  d[0] = d[1] = d[2] = d[3] = 0u;
  if (row >= H) return;
  const uint16_t* p = plane + (size_t)row * W;
  if (VEC) {
    const int c = c0 + lane * kPjCols;
    if (c < W) {  // W % 8 == 0: a vector that starts inside the row ends inside it
      const pj_u32x4 v = *reinterpret_cast<const pj_u32x4*>(p + c);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPjCols; ++j) {
      const int c = c0 + lane + 64 * j;
      const unsigned x = c < W ? (unsigned)p[c] : 0u;
      d[j >> 1] |= x << (16 * (j & 1));
    }
  }
}

// grid (strips(W), tiles(H)), kPjThreads threads.  VEC needs W % 8 == 0 and v, max_z, sum_z 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kPjThreads, 2) void k_project_u16(const uint16_t* __restrict__ v, int Z, int H, int W,
                                                               uint16_t* __restrict__ max_z,
                                                               unsigned long long* __restrict__ sum_z, int first,
                                                               Partials part) {
  __shared__ unsigned l_sum[2][kPjWaves][kPjCols * kPjPitch];
  __shared__ unsigned l_max[2][kPjWaves][kPjCols / 2 * kPjPitch];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: row pointers stay scalar)
  const int S = gridDim.x, T = gridDim.y, s = blockIdx.x, t = blockIdx.y;
  const int c0 = s * kPjStrip, r0 = t * kPjTileRows + wave * kPjRows;
  const size_t plane = (size_t)H * W;
  // the column this thread folds for the tile's y partial, and where its values lie in a wave's LDS rows
  const int q = threadIdx.x;
  const int q_lane = VEC ? q >> 3 : q & 63, q_j = VEC ? q & 7 : q >> 6;

  unsigned zs[kPjRows][kPjCols], zm[kPjRows][kPjCols / 2];
#pragma unroll
  for (int i = 0; i < kPjRows; ++i) {
#pragma unroll
    for (int j = 0; j < kPjCols; ++j) zs[i][j] = 0u;
#pragma unroll
    for (int k = 0; k < kPjCols / 2; ++k) zm[i][k] = 0u;
  }

  // y, second half: this thread's column of plane z from the 8 waves' LDS rows to the tile's partial
  auto fold_y = [&](int z) {
    unsigned ys = 0u, ym = 0u;
#pragma unroll
    for (int w = 0; w < kPjWaves; ++w) {
      ys += l_sum[z & 1][w][q_j * kPjPitch + q_lane];
      ym = pk_max(ym, l_max[z & 1][w][(q_j >> 1) * kPjPitch + q_lane]);
    }
    const int c = c0 + q;
    if (c < W) {
      const size_t at = ((size_t)z * T + t) * W + c;
      part.ysum[at] = ys;
      part.ymax[at] = (uint16_t)((q_j & 1) ? ym >> 16 : ym & 0xffffu);
    }
  };

  unsigned cur[kPjRows][4];
#pragma unroll
  for (int i = 0; i < kPjRows; ++i) load_row<VEC>(v, r0 + i, H, W, c0, lane, cur[i]);
  for (int z = 0; z < Z; ++z) {
    unsigned nxt[kPjRows][4];  // the next plane's loads are issued before this plane is reduced
#pragma unroll
    for (int i = 0; i < kPjRows; ++i)
      load_row<VEC>(v + (size_t)(z + 1) * plane, z + 1 < Z ? r0 + i : H, H, W, c0, lane, nxt[i]);
    // while the loads fly: plane z - 1 of the y reduction.  Buffer z & 1 is written below, behind this barrier, which
    // every thread reaches after it has read that buffer for plane z - 2.
    if (z > 0) {
      lds_barrier();
      fold_y(z - 1);
    }

    unsigned cs[kPjCols], cm[kPjCols / 2];
#pragma unroll
    for (int j = 0; j < kPjCols; ++j) cs[j] = 0u;
#pragma unroll
    for (int k = 0; k < kPjCols / 2; ++k) cm[k] = 0u;
    unsigned rs[kPjRows], rm[kPjRows];
#pragma unroll
    for (int i = 0; i < kPjRows; ++i) {
      rs[i] = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned lo = cur[i][k] & 0xffffu, hi = cur[i][k] >> 16;
        zs[i][2 * k] += lo;
        zs[i][2 * k + 1] += hi;
        cs[2 * k] += lo;
        cs[2 * k + 1] += hi;
        rs[i] += lo + hi;
        zm[i][k] = pk_max(zm[i][k], cur[i][k]);
        cm[k] = pk_max(cm[k], cur[i][k]);
      }
      const unsigned m = pk_max(pk_max(cur[i][0], cur[i][1]), pk_max(cur[i][2], cur[i][3]));
      rm[i] = max(m & 0xffffu, m >> 16);
    }
    // x: the four rows across the 64 lanes in one butterfly -- the upper half of the wave takes rows 2 and 3 and the
    // lower half rows 0 and 1, then each quarter one row: lane 16 r ends with row r (7 exchanges per value, not 24)
    {
      const bool up = lane & 32, odd = lane & 16;
      unsigned s2[2], m2[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        s2[n] = (up ? rs[n + 2] : rs[n]) + (unsigned)__shfl_xor((int)(up ? rs[n] : rs[n + 2]), 32);
        m2[n] = max(up ? rm[n + 2] : rm[n], (unsigned)__shfl_xor((int)(up ? rm[n] : rm[n + 2]), 32));
      }
      unsigned s1 = (odd ? s2[1] : s2[0]) + (unsigned)__shfl_xor((int)(odd ? s2[0] : s2[1]), 16);
      unsigned m1 = max(odd ? m2[1] : m2[0], (unsigned)__shfl_xor((int)(odd ? m2[0] : m2[1]), 16));
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        s1 += (unsigned)__shfl_xor((int)s1, off);
        m1 = max(m1, (unsigned)__shfl_xor((int)m1, off));
      }
      const int r = r0 + (lane >> 4);
      if ((lane & 15) == 0 && r < H) {
        const size_t at = ((size_t)z * S + s) * H + r;
        part.xsum[at] = s1;
        part.xmax[at] = (uint16_t)m1;
      }
    }
    // y, first half: a lane's column values of its 4 rows into the wave's LDS rows
    unsigned* ls = l_sum[z & 1][wave];
    unsigned* lm = l_max[z & 1][wave];
#pragma unroll
    for (int j = 0; j < kPjCols; ++j) ls[j * kPjPitch + lane] = cs[j];
#pragma unroll
    for (int k = 0; k < kPjCols / 2; ++k) lm[k * kPjPitch + lane] = cm[k];
#pragma unroll
    for (int i = 0; i < kPjRows; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) cur[i][k] = nxt[i][k];
    }
  }
  if (Z > 0) {
    lds_barrier();
    fold_y(Z - 1);
  }

  // z: the tile's 32 x 512 maxima and sums, once
#pragma unroll
  for (int i = 0; i < kPjRows; ++i) {
    const int r = r0 + i;
    if (r >= H) continue;
    uint16_t* mz = max_z + (size_t)r * W;
    unsigned long long* sz = sum_z + (size_t)r * W;
    if (VEC) {
      const int c = c0 + lane * kPjCols;
      if (c >= W) continue;
      pj_u32x4 m = {zm[i][0], zm[i][1], zm[i][2], zm[i][3]};
      pj_u64x2 a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = pj_u64x2{zs[i][2 * k], zs[i][2 * k + 1]};
      if (!first) {
        const pj_u32x4 old = *reinterpret_cast<const pj_u32x4*>(mz + c);
        m = pj_u32x4{pk_max(m.x, old.x), pk_max(m.y, old.y), pk_max(m.z, old.z), pk_max(m.w, old.w)};
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += reinterpret_cast<const pj_u64x2*>(sz + c)[k];
      }
      *reinterpret_cast<pj_u32x4*>(mz + c) = m;
#pragma unroll
      for (int k = 0; k < 4; ++k) reinterpret_cast<pj_u64x2*>(sz + c)[k] = a[k];
    } else {
#pragma unroll
      for (int j = 0; j < kPjCols; ++j) {
        const int c = c0 + lane + 64 * j;
        if (c >= W) continue;
        unsigned m = (j & 1) ? zm[i][j >> 1] >> 16 : zm[i][j >> 1] & 0xffffu;
        unsigned long long a = zs[i][j];
        if (!first) {
          m = max(m, (unsigned)mz[c]);
          a += sz[c];
        }
        mz[c] = (uint16_t)m;
        sz[c] = a;
      }
    }
  }
}

// One thread per element of a row pair: e < W folds the tiles of column e into row z_off + z of the y arrays, e >= W
// the strips of row e - W into the x arrays.  grid: any; the threads stride over Z (W + H) elements.
__global__ __launch_bounds__(256) void k_project_fold(int Z, int H, int W, int S, int T, Partials part,
                                                      uint16_t* __restrict__ max_y, unsigned* __restrict__ sum_y,
                                                      uint16_t* __restrict__ max_x, unsigned* __restrict__ sum_x,
                                                      int z_off) {
  const size_t per_z = (size_t)W + H, n = (size_t)Z * per_z;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t z = i / per_z;
    const int e = (int)(i - z * per_z);
    unsigned s = 0u, m = 0u;
    if (e < W) {
#pragma unroll 8
      for (int t = 0; t < T; ++t) {  // (independent loads: eight pairs in flight)
        const size_t at = (z * T + t) * W + e;
        s += part.ysum[at];
        m = max(m, (unsigned)part.ymax[at]);
      }
      sum_y[(z_off + z) * W + e] = s;
      max_y[(z_off + z) * W + e] = (uint16_t)m;
    } else {
      const int h = e - W;
#pragma unroll 8
      for (int k = 0; k < S; ++k) {
        const size_t at = (z * S + k) * H + h;
        s += part.xsum[at];
        m = max(m, (unsigned)part.xmax[at]);
      }
      sum_x[(z_off + z) * H + h] = s;
      max_x[(z_off + z) * H + h] = (uint16_t)m;
    }
  }
}

}  // namespace pj
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_PROJECT_H */
