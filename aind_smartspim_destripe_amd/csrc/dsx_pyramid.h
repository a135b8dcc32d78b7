// dsx_pyramid.h -- the multiscale pyramid of a filtered block, computed where the block lies, gfx950.
//
//   k_pyramid_block : reads the dense [Z, H, W] uint16 block once and writes level 1 and level 2 of the pyramid
//       (compute_pyramid, zarr_destriper.py:365-407; level loop of compute_multiscale, :746-782) straight into Zarr
//       chunk ("brick") order at a z offset inside each level's chunk row -- k_downsample2 twice plus
//       k_planes_to_bricks twice, without the intermediate volumes.  Level 2 is the mean of the TRUNCATED level-1
//       values, which a thread holds in registers.  On request level 2 is also left dense for the levels below.
//   k_pyramid_bricks : the same from a block that is still in the chunk order it was stored in (the stand-alone pyramid
//       of a finished store: a decoded level-0 block), without k_bricks_to_planes in front.
//   k_pyramid_level : one further level (>= 3; under 0.2 % of the bytes) from the dense previous one: 2 x 2 x 2 mean,
//       brick-order store, dense copy for the next level.
//   k_pyramid_step<FZ, FY, FX> : one level of a pyramid with another window (factor 1 or 2 per axis, anisotropic
//       volumes: compute_pyramid(scale_axis=...), compute_multiscale(scale_factor=...)) from the previous one, dense or
//       in chunk order; one launch per level, every level >= 1 but the last also left dense.
//
// Pure HBM streaming like dsx_retile.h: 16-byte loads per lane, row / plane indices from blockIdx, non-temporal
// accesses, no LDS.  A thread of k_pyramid_block owns 4 planes x 4 rows x 8 columns of level 0 = 2 x 2 x 4 level-1
// voxels = 2 level-2 voxels and walks them one z-pair at a time (8 loads in flight), carrying the level-1 sums.
// Brick positions outside the level's volume are not written: the caller zeroes a chunk row before its first block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsx_pyramid_geom.h"
#include "dsx_retile.h"

namespace dsx {

struct PyrBlockArgs {
  const uint16_t* src;
  int Z, H, W;        // dense block (level 0)
  pyr::Level l1, l2;  // l2.Z == 0: level 1 only; l2.bricks may be NULL when only the dense copy is wanted
  uint16_t* dense2;   // nullable: level 2 of the block, dense [l2.Z][l2.H][l2.W]
};

// grid: (ceil(ceil(W1 / 4) / 256), ceil(H1 / 2), ceil(Z1 / 2)); one thread per 4 level-1 voxels of 2 rows x 2 planes.
// VEC == true needs W % 8 == 0, l1.cx % 4 == 0, l2.cx % 2 == 0 and 16 / 8 / 4-byte aligned src / level-1 / level-2
// pointers; otherwise scalar accesses with per-voxel bounds (the tail path, like k_downsample2<false>).
template <bool VEC>
__global__ __launch_bounds__(256) void k_pyramid_block(PyrBlockArgs a) {
  const int xq = blockIdx.x * 256 + threadIdx.x;
  const int x1 = xq * 4;
  if (x1 >= a.l1.W) return;
  const int y2 = blockIdx.y, z2 = blockIdx.z;
  const size_t row = (size_t)a.W, slab = (size_t)a.H * a.W;
  const int n1 = VEC ? 4 : min(4, a.l1.W - x1);
  uint32_t acc[2] = {0, 0};  // sums of the 8 truncated level-1 values under each level-2 voxel
#pragma unroll 1
  for (int dz = 0; dz < 2; ++dz) {
    const int z1 = 2 * z2 + dz;
    if (z1 >= a.l1.Z) break;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int y1 = 2 * y2 + dy;
      if (y1 >= a.l1.H) continue;
      const uint16_t* p = a.src + (size_t)(2 * z1) * slab + (size_t)(2 * y1) * row + 2 * x1;
      uint16_t* d = a.l1.bricks + pyr::brick_offset(a.l1, a.l1.z0 + z1, y1, x1);
      uint32_t s[4] = {0, 0, 0, 0};
      if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + (k >> 1) * slab + (k & 1) * row));
          s[0] += pair_sum(v.x); s[1] += pair_sum(v.y); s[2] += pair_sum(v.z); s[3] += pair_sum(v.w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = pyr::mean8(s[i]);
        u32x2 o;
        o.x = s[0] | (s[1] << 16);
        o.y = s[2] | (s[3] << 16);
        __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(d));
      } else {
        for (int i = 0; i < n1; ++i) {
          uint32_t t = 0;
          for (int k = 0; k < 4; ++k) {
            const uint16_t* q = p + (k >> 1) * slab + (k & 1) * row + 2 * i;
            t += (uint32_t)q[0] + q[1];
          }
          s[i] = pyr::mean8(t);
          a.l1.bricks[pyr::brick_offset(a.l1, a.l1.z0 + z1, y1, x1 + i)] = (uint16_t)s[i];
        }
      }
      acc[0] += s[0] + s[1];
      acc[1] += s[2] + s[3];
    }
  }
  if (z2 >= a.l2.Z || y2 >= a.l2.H) return;
  const int x2 = xq * 2;
  const uint32_t o0 = pyr::mean8(acc[0]), o1 = pyr::mean8(acc[1]);
  if (VEC) {
    const uint32_t o = o0 | (o1 << 16);
    if (a.l2.bricks)
      __builtin_nontemporal_store(o, reinterpret_cast<uint32_t*>(a.l2.bricks + pyr::brick_offset(a.l2, a.l2.z0 + z2, y2, x2)));
    if (a.dense2)
      __builtin_nontemporal_store(o, reinterpret_cast<uint32_t*>(a.dense2 + ((size_t)z2 * a.l2.H + y2) * a.l2.W + x2));
  } else {
    const uint32_t o[2] = {o0, o1};
    for (int i = 0; i < 2 && x2 + i < a.l2.W; ++i) {
      if (a.l2.bricks) a.l2.bricks[pyr::brick_offset(a.l2, a.l2.z0 + z2, y2, x2 + i)] = (uint16_t)o[i];
      if (a.dense2) a.dense2[((size_t)z2 * a.l2.H + y2) * a.l2.W + x2 + i] = (uint16_t)o[i];
    }
  }
}

struct PyrBricksArgs {
  pyr::BrickSrc src;  // the block in the chunk order of the array it was read from
  int Z, H, W;        // its extent (level 0): nothing outside it is read
  pyr::Level l1, l2;  // as PyrBlockArgs
  uint16_t* dense2;
};

// k_pyramid_block for a block that is still in chunk order (a decoded level-0 block of the stand-alone pyramid): same
// grid, same arithmetic, same stores; only the 4 planes x 4 rows x 8 columns of a thread come out of source bricks.
// The offset of a voxel is a plane part + a row part + a column part (dsx_pyramid_geom.h): the column is split once per
// thread, the 4 rows once per thread (from blockIdx.y: scalar registers), the 2 planes of a z pair once per pair.
// VEC == true needs what k_pyramid_block<true> needs and src.cx % 8 == 0: the 8 columns of a thread then lie in one
// brick, 16-byte aligned, and inside [Z, H, W] (W % 8 == 0).  Otherwise scalar accesses with per-voxel bounds.
template <bool VEC>
__global__ __launch_bounds__(256) void k_pyramid_bricks(PyrBricksArgs a) {
  const int xq = blockIdx.x * 256 + threadIdx.x;
  const int x1 = xq * 4;
  if (x1 >= a.l1.W) return;
  const int y2 = blockIdx.y, z2 = blockIdx.z;
  const int n1 = VEC ? 4 : min(4, a.l1.W - x1);
  const uint16_t* base = a.src.bricks + (VEC ? pyr::src_col(a.src, 2 * x1) : 0);
  size_t rows[4];  // rows 4 * y2 .. + 3 (those past 2 * l1.H are not used)
#pragma unroll
  for (int r = 0; r < 4; ++r) rows[r] = pyr::src_row(a.src, 4 * y2 + r);
  uint32_t acc[2] = {0, 0};  // sums of the 8 truncated level-1 values under each level-2 voxel
#pragma unroll 1
  for (int dz = 0; dz < 2; ++dz) {
    const int z1 = 2 * z2 + dz;
    if (z1 >= a.l1.Z) break;
    const size_t planes[2] = {pyr::src_plane(a.src, 2 * z1), pyr::src_plane(a.src, 2 * z1 + 1)};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int y1 = 2 * y2 + dy;
      if (y1 >= a.l1.H) continue;
      uint32_t s[4] = {0, 0, 0, 0};
      if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint16_t* p = base + planes[k >> 1] + rows[2 * dy + (k & 1)];
          const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
          s[0] += pair_sum(v.x); s[1] += pair_sum(v.y); s[2] += pair_sum(v.z); s[3] += pair_sum(v.w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = pyr::mean8(s[i]);
        u32x2 o;
        o.x = s[0] | (s[1] << 16);
        o.y = s[2] | (s[3] << 16);
        __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(a.l1.bricks + pyr::brick_offset(a.l1, a.l1.z0 + z1, y1, x1)));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i >= n1) break;
          const size_t c0 = pyr::src_col(a.src, 2 * (x1 + i)), c1 = pyr::src_col(a.src, 2 * (x1 + i) + 1);
          uint32_t t = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint16_t* q = base + planes[k >> 1] + rows[2 * dy + (k & 1)];
            t += (uint32_t)q[c0] + q[c1];
          }
          s[i] = pyr::mean8(t);
          a.l1.bricks[pyr::brick_offset(a.l1, a.l1.z0 + z1, y1, x1 + i)] = (uint16_t)s[i];
        }
      }
      acc[0] += s[0] + s[1];
      acc[1] += s[2] + s[3];
    }
  }
  if (z2 >= a.l2.Z || y2 >= a.l2.H) return;
  const int x2 = xq * 2;
  const uint32_t o0 = pyr::mean8(acc[0]), o1 = pyr::mean8(acc[1]);
  if (VEC) {
    const uint32_t o = o0 | (o1 << 16);
    if (a.l2.bricks)
      __builtin_nontemporal_store(o, reinterpret_cast<uint32_t*>(a.l2.bricks + pyr::brick_offset(a.l2, a.l2.z0 + z2, y2, x2)));
    if (a.dense2)
      __builtin_nontemporal_store(o, reinterpret_cast<uint32_t*>(a.dense2 + ((size_t)z2 * a.l2.H + y2) * a.l2.W + x2));
  } else {
    const uint32_t o[2] = {o0, o1};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (x2 + i >= a.l2.W) break;
      if (a.l2.bricks) a.l2.bricks[pyr::brick_offset(a.l2, a.l2.z0 + z2, y2, x2 + i)] = (uint16_t)o[i];
      if (a.dense2) a.dense2[((size_t)z2 * a.l2.H + y2) * a.l2.W + x2 + i] = (uint16_t)o[i];
    }
  }
}

struct PyrLevelArgs {
  const uint16_t* src;  // dense previous level of the block
  int Y, X;             // its rows / columns
  pyr::Level out;
  uint16_t* dense;      // nullable: this level dense, for the next one
};

// grid: (ceil(W / 256), H, Z) of the output level; one thread per output voxel.
__global__ __launch_bounds__(256) void k_pyramid_level(PyrLevelArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= a.out.W) return;
  const int y = blockIdx.y, z = blockIdx.z;
  const size_t row = (size_t)a.X, slab = (size_t)a.Y * a.X;
  const uint16_t* p = a.src + (size_t)(2 * z) * slab + (size_t)(2 * y) * row + 2 * x;
  uint32_t t = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint16_t* q = p + (k >> 1) * slab + (k & 1) * row;
    t += (uint32_t)q[0] + q[1];
  }
  const uint16_t v = (uint16_t)pyr::mean8(t);
  a.out.bricks[pyr::brick_offset(a.out, a.out.z0 + z, y, x)] = v;
  if (a.dense) a.dense[((size_t)z * a.out.H + y) * a.out.W + x] = v;
}

struct PyrStepArgs {
  const uint16_t* src;  // BRICKS == false: the dense previous level [..][Y][X]
  pyr::BrickSrc bsrc;   // BRICKS == true: the previous level (level 0 of a block) in chunk order
  int Y, X;             // rows / columns of the previous level
  pyr::Level out;       // this level; out.bricks may be NULL when only the dense copy is wanted
  uint16_t* dense;      // nullable: this level dense [out.Z][out.H][out.W], for the next one
};

// One level of a pyramid with an FZ x FY x FX window (a pyr::Scale other than 2 x 2 x 2) from the previous one: mean,
// brick-order store at out.z0, dense copy for the next level.  A thread owns 8 source columns of FZ planes x FY rows
// (one 16-byte load each) = N = 8 / FX output voxels of one row (one 8- or 16-byte store).
// grid: (ceil(ceil(out.W / N) / 256), out.H, out.Z).
// VEC == true needs X % 8 == 0, out.cx % N == 0, a 16-byte aligned source (bsrc.cx % 8 == 0 for bricks) and 2 N-byte
// aligned outputs; otherwise scalar accesses with per-voxel bounds (the tail body).
template <int FZ, int FY, int FX, bool VEC, bool BRICKS>
__global__ __launch_bounds__(256) void k_pyramid_step(PyrStepArgs a) {
  constexpr int N = 8 / FX;
  constexpr int SHIFT = (FZ - 1) + (FY - 1) + (FX - 1);
  const int x = (blockIdx.x * 256 + threadIdx.x) * N;
  if (x >= a.out.W) return;
  const int y = blockIdx.y, z = blockIdx.z;
  const size_t dense_at = ((size_t)z * a.out.H + y) * a.out.W + x;
  if (VEC) {
    uint32_t s[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = 0;
    const size_t col = BRICKS ? pyr::src_col(a.bsrc, FX * x) : (size_t)(FX * x);
#pragma unroll
    for (int dz = 0; dz < FZ; ++dz) {
#pragma unroll
      for (int dy = 0; dy < FY; ++dy) {
        const int zs = FZ * z + dz, ys = FY * y + dy;
        const uint16_t* p = BRICKS ? a.bsrc.bricks + pyr::src_plane(a.bsrc, zs) + pyr::src_row(a.bsrc, ys) + col
                                   : a.src + ((size_t)zs * a.Y + ys) * a.X + col;
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        if constexpr (FX == 2) {
          s[0] += pair_sum(v.x); s[1] += pair_sum(v.y); s[2] += pair_sum(v.z); s[3] += pair_sum(v.w);
        } else {
          s[0] += v.x & 0xffffu; s[1] += v.x >> 16; s[2] += v.y & 0xffffu; s[3] += v.y >> 16;
          s[4] += v.z & 0xffffu; s[5] += v.z >> 16; s[6] += v.w & 0xffffu; s[7] += v.w >> 16;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = pyr::window_mean(s[i], SHIFT);
    using V = typename U16Vec<N>::type;
    V o;
    o.x = s[0] | (s[1] << 16);
    o.y = s[2] | (s[3] << 16);
    if constexpr (N == 8) {
      o.z = s[4] | (s[5] << 16);
      o.w = s[6] | (s[7] << 16);
    }
    if (a.out.bricks)
      __builtin_nontemporal_store(o, reinterpret_cast<V*>(a.out.bricks + pyr::brick_offset(a.out, a.out.z0 + z, y, x)));
    if (a.dense) __builtin_nontemporal_store(o, reinterpret_cast<V*>(a.dense + dense_at));
  } else {
    const pyr::DenseAt dense = {a.src, (size_t)a.Y * a.X, (size_t)a.X};
    const pyr::BrickAt bricks = {a.bsrc};
    for (int i = 0; i < N && x + i < a.out.W; ++i) {
      const uint32_t t = BRICKS ? pyr::window_sum(bricks, z, y, x + i, FZ, FY, FX) : pyr::window_sum(dense, z, y, x + i, FZ, FY, FX);
      const uint16_t v = (uint16_t)pyr::window_mean(t, SHIFT);
      if (a.out.bricks) a.out.bricks[pyr::brick_offset(a.out, a.out.z0 + z, y, x + i)] = v;
      if (a.dense) a.dense[dense_at + i] = v;
    }
  }
}

// The body of k_pyramid_step<FZ, FY, FX> that the geometry allows (dsx.hip decides `vec`).
template <int FZ, int FY, int FX>
inline void launch_pyramid_step(bool vec, bool bricks, const dim3& grid, hipStream_t s, const PyrStepArgs& a) {
  if (vec && bricks) hipLaunchKernelGGL((k_pyramid_step<FZ, FY, FX, true, true>), grid, dim3(256), 0, s, a);
  else if (vec) hipLaunchKernelGGL((k_pyramid_step<FZ, FY, FX, true, false>), grid, dim3(256), 0, s, a);
  else if (bricks) hipLaunchKernelGGL((k_pyramid_step<FZ, FY, FX, false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_pyramid_step<FZ, FY, FX, false, false>), grid, dim3(256), 0, s, a);
}

}  // namespace dsx
