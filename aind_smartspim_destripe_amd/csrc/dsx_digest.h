// dsx_digest.h -- per-chunk content digests of uint16 bricks in chunk order (gfx950), and their host build.
//
// A store pass deletes its input once the destriped store exists, and neither the Blosc frames nor the zstd frames it
// writes carry a checksum: a chunk that decodes to the wrong voxels raises nothing.  At the moment a chunk is written
// its voxels lie in device memory in chunk order (the output of k_planes_to_bricks, the rows of k_pyramid_block /
// k_pyramid_step, the output of the decoders), so one more streaming read gives a record per chunk that a later pass
// over the store can recompute and compare (integrity.py).  The records go to a sidecar; the store's bytes do not change.
//
// The contract is exact integer arithmetic mod 2^64, so the kernel, the host build and a NumPy uint64 restatement are
// compared for EQUALITY.  For a chunk (c0, c1, c2) with valid extents (e0, e1, e2) -- the part inside the array; what a
// stored brick holds in its padding never enters -- and the valid voxel v at local (i0, i1, i2), row r = i0 * c1 + i1
// (the row index of the FULL chunk, so a voxel's weight does not depend on the extents):
//
//   m(k)  : z = (k + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
//           z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  m = (z ^ (z >> 31)) | 1         (splitmix64's output, made odd)
//   count = e0 * e1 * e2
//   sum   = SUM v
//   wsum  = SUM_r  m(r) * ( SUM_{i2 < e2}  v[r, i2] * m(2^32 + i2) )
//
// A record is (count, sum, wsum), three uint64.  Every weight m(r) * m(2^32 + i2) is odd, hence invertible mod 2^64:
// changing one voxel by d, 0 < |d| < 2^16, changes wsum by d * (odd) != 0.  The digest is not cryptographic: it is
// built to catch torn writes, swapped or stale files, flipped bits and encoder faults, not an adversary.
//
// The weight is a product of a row weight and a column weight so that a lane which owns fixed columns keeps its eight
// column weights in registers: per 8 voxels it pays eight 16 x 64-bit multiply-adds and ONE 64 x 64-bit multiply by the
// row weight.  (64-bit integer multiplies are several quarter-rate 32-bit ones on this chip; a splitmix per voxel would
// make the kernel VALU-bound several times over.)  The row weights of a block's rows are computed once, into LDS.
//
//   k_brick_digest_u16 : a grid of (n0, n1, n2) bricks of (c0, c1, c2) voxels, back to back in C order of the grid, and
//       (v0, v1, v2), the valid voxels the buffer covers along each axis from its chunk-aligned origin: brick g has
//       extents min(c_a, v_a - g_a * c_a).  One block of 256 threads per (brick, segment of kDgSegRows rows).  The
//       block is LX lanes along the row (LX the power of two that covers the row's 8-voxel vectors, at most 256) by
//       256 / LX rows; a lane walks the segment's rows in steps of 256 / LX with kDgUnroll loads in flight, and rows
//       wider than 2048 voxels in several column passes.  What lies outside the extents is inside the buffer (bricks
//       are stored whole), so no load depends on a condition and the kDgUnroll loads of a lane leave back to back; a
//       row outside the extents has LDS weight 0 (which no real weight is) and is left out of the sum, columns outside
//       are masked, vectors wholly outside are not visited, and a segment behind the last valid plane exits at once.
//       VEC = true: c2 % 8 == 0 and a 16-byte aligned base, so every row starts on a 16-byte boundary: one 16-byte load
//       per 8 voxels; the ragged end of a row of an edge brick is a whole in-bounds vector whose tail is masked.
//       VEC = false (any c2, any 2-byte aligned base): eight 2-byte loads, those past the extent re-reading its last
//       column.
//       Lane sums are 64-bit; a wave reduction (shuffles), a block reduction (LDS), then one 64-bit atomic add per block
//       and field into the records, which the launch zeroes first.  Integer adds commute: the result is exact in any
//       order.  No scratch, 4.2 KiB of LDS.
//   chunk_digest_host / grid_digest_host : the same records on the host (dsx_brick_digest_u16_ref), plain C++.
#ifndef DSX_DIGEST_H
#define DSX_DIGEST_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define DSX_DG_HD __host__ __device__ __forceinline__
#else
#define DSX_DG_HD inline
#endif

namespace dsx {
namespace dg {

constexpr int kDgThreads = 256;
constexpr int kDgSegRows = 512;                   // rows of a brick per block: 4 KiB of row weights in LDS
constexpr int kDgUnroll = 4;                      // loads in flight per lane
constexpr int kDgRecord = 3;                      // uint64 per record: count, sum, wsum
constexpr uint64_t kDgColBase = 1ull << 32;       // column i2 has weight m(2^32 + i2)
constexpr int64_t kDgMaxBrick = (int64_t)1 << 31;  // voxels per brick
constexpr int kDgMaxRow = 1 << 30;                // voxels per row (the column index stays an int with room to step)
constexpr int64_t kDgMaxBlocks = 0x7fffffff;      // blocks of one launch

// m(k): splitmix64's output function over (k + 1) * golden gamma, made odd.
DSX_DG_HD uint64_t weight(uint64_t k) {
  uint64_t z = (k + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (z ^ (z >> 31)) | 1ull;
}

// Valid voxels of brick g along an axis of chunk c where the buffer covers v voxels: min(c, v - g * c).
DSX_DG_HD int extent(int c, int v, int g) {
  const int64_t left = (int64_t)v - (int64_t)g * c;
  return (int)(left < c ? left : c);
}

struct Geometry {
  int lx;         // lanes along a row (power of two, <= kDgThreads)
  int ly;         // rows in flight per block: kDgThreads / lx
  int64_t rows;   // rows of a brick: c0 * c1
  int64_t segs;   // blocks per brick
  int64_t grid;   // blocks of the launch
};

// The launch geometry of (n0 * n1 * n2) bricks of (c0, c1, c2) voxels.  The caller has checked the arguments.
inline Geometry geometry(int64_t bricks, int c0, int c1, int c2) {
  Geometry g;
  const int nvec = (int)(((int64_t)c2 + 7) / 8);
  g.lx = 1;
  while (g.lx < nvec && g.lx < kDgThreads) g.lx *= 2;
  g.ly = kDgThreads / g.lx;
  g.rows = (int64_t)c0 * c1;
  g.segs = (g.rows + kDgSegRows - 1) / kDgSegRows;
  g.grid = bricks * g.segs;
  return g;
}

// NULL when the geometry can be digested, otherwise what is wrong with it.
inline const char* check_geometry(int n0, int n1, int n2, int c0, int c1, int c2, int v0, int v1, int v2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return "digest: the brick grid must not be empty";
  if (c0 < 1 || c1 < 1 || c2 < 1) return "digest: chunk shapes must be positive";
  const int64_t rows = (int64_t)c0 * c1;
  if (rows > kDgMaxBrick || rows * c2 > kDgMaxBrick) return "digest: a brick holds more than 2^31 voxels";
  if (c2 > kDgMaxRow) return "digest: a row holds more than 2^30 voxels";
  const int n[3] = {n0, n1, n2}, c[3] = {c0, c1, c2}, v[3] = {v0, v1, v2};
  for (int a = 0; a < 3; ++a)  // every brick of the grid holds at least one valid voxel, and no voxel lies outside it
    if ((int64_t)v[a] <= (int64_t)(n[a] - 1) * c[a] || (int64_t)v[a] > (int64_t)n[a] * c[a])
      return "digest: the valid extents do not end inside the last brick of each axis";
  const int64_t bricks = (int64_t)n0 * n1;
  if (bricks > kDgMaxBlocks || bricks * n2 > kDgMaxBlocks) return "digest: too many bricks";
  const Geometry g = geometry(bricks * n2, c0, c1, c2);
  if (g.grid > kDgMaxBlocks) return "digest: too many blocks for one launch";
  return nullptr;
}

// The record of one brick: c = chunk shape, e = valid extents (1 <= e_a <= c_a), out = {count, sum, wsum}.
inline void chunk_digest_host(const uint16_t* brick, const int c[3], const int e[3], uint64_t out[3]) {
  uint64_t sum = 0, wsum = 0;
  for (int i0 = 0; i0 < e[0]; ++i0)
    for (int i1 = 0; i1 < e[1]; ++i1) {
      const uint64_t r = (uint64_t)i0 * (uint64_t)c[1] + (uint64_t)i1;
      const uint16_t* row = brick + (size_t)r * (size_t)c[2];
      uint64_t dot = 0;
      for (int i2 = 0; i2 < e[2]; ++i2) {
        sum += row[i2];
        dot += (uint64_t)row[i2] * weight(kDgColBase + (uint64_t)i2);
      }
      wsum += weight(r) * dot;
    }
  out[0] = (uint64_t)e[0] * (uint64_t)e[1] * (uint64_t)e[2];
  out[1] = sum;
  out[2] = wsum;
}

// The records of a grid of bricks (the kernel's arguments), out[n0 * n1 * n2][3].
inline void grid_digest_host(const uint16_t* bricks, int n0, int n1, int n2, int c0, int c1, int c2, int v0, int v1,
                             int v2, uint64_t* out) {
  const int c[3] = {c0, c1, c2};
  const size_t brick = (size_t)c0 * (size_t)c1 * (size_t)c2;
  size_t b = 0;
  for (int g0 = 0; g0 < n0; ++g0)
    for (int g1 = 0; g1 < n1; ++g1)
      for (int g2 = 0; g2 < n2; ++g2, ++b) {
        const int e[3] = {extent(c0, v0, g0), extent(c1, v1, g1), extent(c2, v2, g2)};
        chunk_digest_host(bricks + b * brick, c, e, out + b * kDgRecord);
      }
}

}  // namespace dg
}  // namespace dsx

#if defined(__HIP__)

namespace dsx {
namespace dg {

typedef unsigned int dg_u32x4 __attribute__((ext_vector_type(4)));

struct DigestArgs {
  const uint16_t* bricks;
  unsigned long long* out;  // [bricks][3], zeroed before the launch
  int n1, n2;
  int c0, c1, c2;
  int v0, v1, v2;
  int lx_log2;              // lanes along a row = 1 << lx_log2
  unsigned segs;            // blocks per brick
};

__device__ __forceinline__ unsigned long long dg_wave_sum(unsigned long long x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
  return x;
}

// The 8 voxels at columns x0 .. x0 + 7 of a row as 4 words of two (x0 < e2; the caller masks the columns >= e2).  No
// load depends on a condition, so the loads of kDgUnroll rows are issued back to back: the vector load reads a whole
// in-bounds vector (c2 % 8 == 0), the 2-byte loads past the extent re-read column e2 - 1.
template <bool VEC>
__device__ __forceinline__ dg_u32x4 dg_load8(const uint16_t* __restrict__ row, int x0, int e2) {
  if (VEC) return *reinterpret_cast<const dg_u32x4*>(row + x0);
  unsigned h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = (unsigned)row[x0 + k < e2 ? x0 + k : e2 - 1];
  return dg_u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}

// grid: bricks * segs blocks of kDgThreads threads, block (b, s) = blockIdx.x / segs, % segs.
template <bool VEC>
__global__ __launch_bounds__(kDgThreads) void k_brick_digest_u16(const DigestArgs a) {
  __shared__ unsigned long long roww[kDgSegRows];
  __shared__ unsigned long long part[2][kDgThreads / 64];

  const unsigned b = blockIdx.x / a.segs, seg = blockIdx.x - b * a.segs;
  const int g2 = (int)(b % (unsigned)a.n2), g1 = (int)((b / (unsigned)a.n2) % (unsigned)a.n1);
  const int g0 = (int)(b / ((unsigned)a.n2 * (unsigned)a.n1));
  const int e0 = extent(a.c0, a.v0, g0), e1 = extent(a.c1, a.v1, g1), e2 = extent(a.c2, a.v2, g2);

  const long long rows = (long long)a.c0 * a.c1;
  const long long r_first = (long long)seg * kDgSegRows;
  // a segment that starts behind the last valid plane of the brick has no valid row (never segment 0, which writes
  // the count): the whole block leaves before it reads anything
  if (r_first / a.c1 >= e0) return;
  const int n_rows = (int)(rows - r_first < kDgSegRows ? rows - r_first : kDgSegRows);
  // row weights of the segment; 0 (which no weight is: they are odd) for the rows outside the extents
  for (int k = threadIdx.x; k < n_rows; k += kDgThreads) {
    const long long r = r_first + k;
    const long long i0 = r / a.c1, i1 = r - i0 * a.c1;
    roww[k] = (i0 < e0 && i1 < e1) ? weight((unsigned long long)r) : 0ull;
  }
  __syncthreads();

  const int lx = 1 << a.lx_log2, ly = kDgThreads >> a.lx_log2;
  const int tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> a.lx_log2;
  const size_t brick = (size_t)rows * (size_t)a.c2;
  const uint16_t* __restrict__ base = a.bricks + (size_t)b * brick + (size_t)r_first * (size_t)a.c2;

  unsigned long long sum = 0ull, wsum = 0ull;
  for (int x0 = tx * 8; x0 < e2; x0 += lx * 8) {  // (one pass unless the row is wider than 2048 voxels)
    unsigned long long cw[8];
    dg_u32x4 mask;
#pragma unroll
    for (int k = 0; k < 8; ++k) cw[k] = weight(kDgColBase + (unsigned long long)(x0 + k));
    mask.x = (x0 + 0 < e2 ? 0xffffu : 0u) | (x0 + 1 < e2 ? 0xffff0000u : 0u);
    mask.y = (x0 + 2 < e2 ? 0xffffu : 0u) | (x0 + 3 < e2 ? 0xffff0000u : 0u);
    mask.z = (x0 + 4 < e2 ? 0xffffu : 0u) | (x0 + 5 < e2 ? 0xffff0000u : 0u);
    mask.w = (x0 + 6 < e2 ? 0xffffu : 0u) | (x0 + 7 < e2 ? 0xffff0000u : 0u);
    for (int r0 = ty; r0 < n_rows; r0 += kDgUnroll * ly) {
      dg_u32x4 w[kDgUnroll];
      unsigned long long rw[kDgUnroll];
#pragma unroll
      for (int u = 0; u < kDgUnroll; ++u) {  // (a step past the segment re-reads its last row with weight 0)
        const int r = r0 + u * ly, rc = r < n_rows ? r : n_rows - 1;
        rw[u] = r < n_rows ? roww[rc] : 0ull;
        w[u] = dg_load8<VEC>(base + (size_t)rc * (size_t)a.c2, x0, e2);
      }
#pragma unroll
      for (int u = 0; u < kDgUnroll; ++u) {
        const unsigned q[4] = {w[u].x & mask.x, w[u].y & mask.y, w[u].z & mask.z, w[u].w & mask.w};
        unsigned long long dot = 0ull;
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned lo = q[k] & 0xffffu, hi = q[k] >> 16;
          s += lo + hi;
          dot += (unsigned long long)lo * cw[2 * k] + (unsigned long long)hi * cw[2 * k + 1];
        }
        sum += rw[u] ? s : 0u;  // (a row outside the extents was read, not counted)
        wsum += rw[u] * dot;
      }
    }
  }

  sum = dg_wave_sum(sum);
  wsum = dg_wave_sum(wsum);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[0][wave] = sum;
    part[1][wave] = wsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0ull, ws = 0ull;
#pragma unroll
    for (int k = 0; k < kDgThreads / 64; ++k) {
      s += part[0][k];
      ws += part[1][k];
    }
    unsigned long long* rec = a.out + (size_t)b * kDgRecord;
    if (seg == 0) atomicAdd(&rec[0], (unsigned long long)e0 * (unsigned long long)e1 * (unsigned long long)e2);
    if (s) atomicAdd(&rec[1], s);
    if (ws) atomicAdd(&rec[2], ws);
  }
}

}  // namespace dg
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_DIGEST_H */
