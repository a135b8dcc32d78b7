// dsx_volhist.h -- exact 65 536-bin histogram of a uint16 volume, accumulated over calls (gfx950), and its host build.
//
// The reference wants the display window of its OME-NGFF metadata to be da.percentile(image_data, (0.1, 95)) and
// hard-codes (0.0, 350.0) because the percentile "would take so much time and resources" (zarr_destriper.py:722-726).
// In the chunk map every filtered voxel of a block lies in device memory as uint16 [Z, H, W] before it is re-tiled, so
// the histogram of the whole output volume costs one more streaming read of those planes, and percentiles of a
// histogram are exact.
//
//   k_volhist_u16 : ONE pass over n contiguous voxels.  The pointer is only 2-byte aligned (callers hand in sub-ranges),
//       so block 0 counts the head up to the first 16-byte boundary and the tail behind the last whole vector with
//       2-byte loads; everything between is read with one 16-byte load per lane (8 voxels), four loads in flight per
//       lane, blocks striding over the vectors.
//
//       Counting: a block owns kVhWin = 16 384 32-bit bins in LDS (64 KiB) for the values 0 .. 16 383.  All 65 536
//       bins would take 256 KiB and a CU has 160 KiB, so the window covers the LOW values: destriped light-sheet data
//       is background of a few hundred counts and tissue of a few thousand (the reference's own window ends at 350),
//       and 64 KiB leaves room for two resident blocks of 512 threads per CU -- 16 waves, enough loads in flight to
//       stream -- where 128 KiB (32 768 bins) would leave one.  A value outside the window goes straight to the global
//       histogram with a 64-bit atomic add; on microscopy data these are the few saturated voxels.  At block end only
//       the non-zero LDS bins are added to the global uint64 bins.  One call counts n < 2^32 voxels (the caller
//       checks), so no 32-bit bin can overflow.
//
//       Contention: destriped background is nearly constant, so many lanes of a wave hit one bin, and LDS atomics to
//       one address serialise.  Two exact pre-aggregations: a lane merges runs of equal values among its 8 voxels into
//       one add of the run length; and when every active lane of a wave holds 8 copies of the same value, lane 0 adds
//       8 x (active lanes) once.  Both only regroup integer additions: the counts are exact whatever the data.
//
//   volhist_host  : the same counts on the host (dsx_volhist_ref), plain C++.
#ifndef DSX_VOLHIST_H
#define DSX_VOLHIST_H

#include <stddef.h>
#include <stdint.h>

namespace dsx {
namespace vh {

constexpr int kVhBins = 65536;   // global histogram: one uint64 per uint16 value
constexpr int kVhWin = 16384;    // values counted in LDS (64 KiB of 32-bit bins per block)
constexpr int kVhThreads = 512;  // two blocks per CU: 2 x 64 KiB of the 160 KiB
constexpr int kVhUnroll = 4;     // 16-byte loads in flight per lane

// hist[v] += number of voxels equal to v
inline void volhist_host(const uint16_t* vox, size_t n, uint64_t* hist) {
  for (size_t i = 0; i < n; ++i) ++hist[vox[i]];
}

// Voxels in front of the first 16-byte boundary (at most 7, at most n); p is 2-byte aligned.
inline size_t head_voxels(const void* p, size_t n) {
  const size_t h = ((16 - ((uintptr_t)p & 15)) & 15) / 2;
  return h < n ? h : n;
}

}  // namespace vh
}  // namespace dsx

#if defined(__HIP__)
#include <hip/hip_runtime.h>

namespace dsx {
namespace vh {

typedef unsigned int vh_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void vh_count(unsigned* win, unsigned long long* hist, unsigned v, unsigned c) {
  if (v < (unsigned)kVhWin) atomicAdd(&win[v], c);
  else atomicAdd(&hist[v], (unsigned long long)c);
}

// grid: any number of blocks of kVhThreads threads (the launch takes two per CU, fewer for short ranges).
// body: the 16-byte aligned part of the range, n_vec vectors of 8 voxels; head / tail: what lies in front of / behind it.
__global__ __launch_bounds__(kVhThreads) void k_volhist_u16(const uint16_t* __restrict__ vox, size_t head, size_t n_vec,
                                                            size_t tail, unsigned long long* __restrict__ hist) {
  __shared__ unsigned win[kVhWin];
  for (int k = threadIdx.x; k < kVhWin; k += kVhThreads) win[k] = 0u;
  __syncthreads();

  if (blockIdx.x == 0) {  // head and tail: fewer than 8 voxels each
    if (threadIdx.x < head) vh_count(win, hist, vox[threadIdx.x], 1u);
    if (threadIdx.x < tail) vh_count(win, hist, vox[head + n_vec * 8 + threadIdx.x], 1u);
  }

  const vh_u32x4* body = reinterpret_cast<const vh_u32x4*>(vox + head);
  const size_t stride = (size_t)gridDim.x * kVhThreads;
  const bool lane0 = (threadIdx.x & 63) == 0;
  // (the loop bound is the same for every thread of a block, so the ballots below see whole waves)
  for (size_t base = (size_t)blockIdx.x * kVhThreads; base < n_vec; base += kVhUnroll * stride) {
    vh_u32x4 v[kVhUnroll];
    bool ok[kVhUnroll];
#pragma unroll
    for (int k = 0; k < kVhUnroll; ++k) {
      const size_t i = base + k * stride + threadIdx.x;
      ok[k] = i < n_vec;
      v[k] = ok[k] ? body[i] : vh_u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < kVhUnroll; ++k) {
      const unsigned x0 = v[k].x & 0xffffu;
      const unsigned rep = x0 | (x0 << 16);
      const bool same = v[k].x == rep && v[k].y == rep && v[k].z == rep && v[k].w == rep;
      // vectors go to lanes in order, so the lanes with a vector are a prefix of the wave: lane 0 has one if any has
      const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)x0);
      const unsigned long long act = __ballot(ok[k]);
      const unsigned long long uni = __ballot(ok[k] && same && x0 == first);
      if (act == 0ull) continue;
      if (uni == act) {  // the whole wave holds one value
        if (lane0) vh_count(win, hist, first, 8u * (unsigned)__popcll(act));
        continue;
      }
      if (!ok[k]) continue;
      const unsigned w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
      unsigned cur = x0, c = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // runs of equal values: one add per run
        const unsigned x = (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu);
        if (x == cur) {
          ++c;
        } else {
          vh_count(win, hist, cur, c);
          cur = x;
          c = 1u;
        }
      }
      vh_count(win, hist, cur, c);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kVhWin; k += kVhThreads) {
    const unsigned c = win[k];
    if (c) atomicAdd(&hist[k], (unsigned long long)c);
  }
}

}  // namespace vh
}  // namespace dsx
#endif  // __HIP__

#endif /* DSX_VOLHIST_H */
