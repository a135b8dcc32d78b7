// dsx_rot90.h -- quarter turns of a batch of planes: [n, H, W] -> [n, W, H], np.rot90(x) (DIR +1) or np.rot90(x, -1)
// (DIR -1) per plane.  What a rotated plan (dsx_set_rotate) puts in front of and behind the launch chain, and
// dsx_rot90_device / dsx_rot90_ref on their own.
//
// The index map, the tile and the launch geometry are pure C++ (no HIP) like dsx_chain.h, so that
// tests/host/dsx_rot90_check.cpp can hold them with g++ and no GPU; the kernel below them is compiled by hipcc only.
#ifndef DSX_ROT90_H
#define DSX_ROT90_H

#include <stddef.h>
#include <stdint.h>

namespace dsx {
namespace rot {

#ifdef __HIPCC__
#define DSX_ROT_HD __host__ __device__
#else
#define DSX_ROT_HD
#endif

constexpr int kRotTile = 64;      // a block moves kRotTile x kRotTile elements: 64 lanes along a row on either side
constexpr int kRotThreads = 256;  // 4 waves, each takes every 4th row of the tile
constexpr unsigned kRotMaxGridZ = 65535u;

// Source element (r, c) of the plane [H, W] that destination element (i, j) of the plane [W, H] takes:
//   dir +1: np.rot90(x)[i, j]     == x[j, W - 1 - i]
//   dir -1: np.rot90(x, -1)[i, j] == x[H - 1 - j, i]
inline DSX_ROT_HD int rot_src_row(int dir, int H, int j) { return dir > 0 ? j : H - 1 - j; }
inline DSX_ROT_HD int rot_src_col(int dir, int W, int i) { return dir > 0 ? W - 1 - i : i; }
// ... and the destination row that source column c lands in (the inverse of rot_src_col)
inline DSX_ROT_HD int rot_dst_row(int dir, int W, int c) { return dir > 0 ? W - 1 - c : c; }

// LDS pitch of a tile row in elements.  The tile is written along its rows and read down its columns: lane k of a
// 32-lane group reads dword k * pitch_dwords + const, and ds_read_b32 / _u16 take the bank as dword mod 32, so an odd
// dword pitch puts the 32 lanes on 32 banks.  float32: 65 dwords.  uint16: two elements share a dword, so the pitch is
// 66 elements = 33 dwords (an element pitch of 65 is 32.5 dwords: rows k and k + 1 would meet on one bank for every
// other column).  The row-wise uint16 writes of phase 1 put two lanes on each dword, at the same dword address.
inline DSX_ROT_HD int rot_pitch(size_t elem_bytes) { return elem_bytes == 2 ? kRotTile + 2 : kRotTile + 1; }
inline size_t rot_lds_bytes(size_t elem_bytes) { return (size_t)kRotTile * rot_pitch(elem_bytes) * elem_bytes; }

// Grid of one launch: x = tiles over the SOURCE columns c (== destination rows), y = tiles over the DESTINATION columns
// j (== source rows, mirrored for dir -1), z = planes.  Both column ranges start at multiples of the tile, so source
// reads and destination writes of a full tile are whole 128-byte (uint16) / 256-byte (float32) runs when the row
// pitches allow; the last tile of either axis is partial.
struct RotGrid {
  unsigned x, y, z;
};
inline RotGrid rot_grid(int n, int H, int W) {
  RotGrid g;
  g.x = (unsigned)((W + kRotTile - 1) / kRotTile);
  g.y = (unsigned)((H + kRotTile - 1) / kRotTile);
  g.z = (unsigned)n;  // callers split n at kRotMaxGridZ
  return g;
}

// One tile element of the two phases, as the kernel and the host check both walk them.  A block (bx, by) covers source
// columns c0 = bx * tile .. and destination columns j0 = by * tile ..; the tile is indexed [j - j0][c - c0].
struct RotElem {
  bool live;      // inside the plane
  size_t src;     // element offset inside the source plane [H, W]
  size_t dst;     // element offset inside the destination plane [W, H]
};
inline DSX_ROT_HD RotElem rot_elem(int dir, int H, int W, unsigned bx, unsigned by, int tj, int tc) {
  const int c = (int)bx * kRotTile + tc, j = (int)by * kRotTile + tj;
  RotElem e;
  e.live = c < W && j < H;
  e.src = e.live ? (size_t)rot_src_row(dir, H, j) * W + c : 0;
  e.dst = e.live ? (size_t)rot_dst_row(dir, W, c) * H + j : 0;
  return e;
}

// Host build of the map: every destination element from its source element.
template <typename T>
inline void rot90_host(const T* src, T* dst, int n, int H, int W, int dir) {
  const size_t px = (size_t)H * W;
  for (int p = 0; p < n; ++p)
    for (int i = 0; i < W; ++i)
      for (int j = 0; j < H; ++j)
        dst[p * px + (size_t)i * H + j] = src[p * px + (size_t)rot_src_row(dir, H, j) * W + rot_src_col(dir, W, i)];
}

#ifdef __HIPCC__
// Phase 1: wave w of the block loads tile rows w, w + 4, ... -- lane = source column, one source row per instruction.
// Phase 2: it stores destination rows (tile columns) w, w + 4, ... -- lane = destination column, one tile column per
// instruction, read down the tile with the pitch above.  No scratch: 32 loop trips over registers, the tile in LDS.
template <typename T, int DIR>
__global__ __launch_bounds__(kRotThreads) void k_rot90(const T* __restrict__ src, T* __restrict__ dst, int H, int W) {
  constexpr int P = sizeof(T) == 2 ? kRotTile + 2 : kRotTile + 1;
  __shared__ T tile[kRotTile * P];
  const size_t px = (size_t)H * W;
  const T* s = src + (size_t)blockIdx.z * px;
  T* d = dst + (size_t)blockIdx.z * px;
  const int lane = threadIdx.x & (kRotTile - 1), w = threadIdx.x / kRotTile;
  constexpr int kStep = kRotThreads / kRotTile;
#pragma unroll 4
  for (int tj = w; tj < kRotTile; tj += kStep) {
    const RotElem e = rot_elem(DIR, H, W, blockIdx.x, blockIdx.y, tj, lane);
    if (e.live) tile[tj * P + lane] = s[e.src];
  }
  __syncthreads();
#pragma unroll 4
  for (int tc = w; tc < kRotTile; tc += kStep) {
    const RotElem e = rot_elem(DIR, H, W, blockIdx.x, blockIdx.y, lane, tc);
    if (e.live) d[e.dst] = tile[lane * P + tc];
  }
}

template <typename T>
inline void rot90_launch(hipStream_t s, const void* src, void* dst, int n, int H, int W, int dir) {
  const size_t px = (size_t)H * W;
  for (int p0 = 0; p0 < n; p0 += (int)kRotMaxGridZ) {
    const int np = n - p0 < (int)kRotMaxGridZ ? n - p0 : (int)kRotMaxGridZ;
    const RotGrid g = rot_grid(np, H, W);
    const T* sp = (const T*)src + (size_t)p0 * px;
    T* dp = (T*)dst + (size_t)p0 * px;
    if (dir > 0) hipLaunchKernelGGL((k_rot90<T, 1>), dim3(g.x, g.y, g.z), dim3(kRotThreads), 0, s, sp, dp, H, W);
    else hipLaunchKernelGGL((k_rot90<T, -1>), dim3(g.x, g.y, g.z), dim3(kRotThreads), 0, s, sp, dp, H, W);
  }
}
#endif  // __HIPCC__

}  // namespace rot
}  // namespace dsx

#endif  // DSX_ROT90_H
