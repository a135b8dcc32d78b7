// dsx_pyramid_geom.h -- window arithmetic and brick addressing of the fused pyramid, shared by the device kernels
// (dsx_pyramid.h) and the host build of the same computation (pyramid_block_host below).  Plain C++.
//
// A block is a dense [Z, H, W] uint16 stack whose first plane lies at a multiple of 2^(levels - 1) in the volume, so
// every 2 x 2 x 2 window of every level lies inside it.  Level l of the block is (Z >> l, H >> l, W >> l): trailing odd
// planes / rows / columns are cropped per level, never averaged.  Every level is the truncated mean of the TRUNCATED
// previous level (compute_pyramid, zarr_destriper.py:365-407: windowed_mean + preserve_dtype), not of level 0.
//
// A Scale (fz, fy, fx), each factor 1 or 2 and not all 1, generalises this (compute_pyramid(scale_axis=...)): the window
// is fz x fy x fx, an axis with factor 1 keeps its extent at every level, the first plane of a block lies at a multiple
// of fz^(levels - 1), and the mean of 2, 4 or 8 voxels is a shift by 1, 2 or 3.
#ifndef DSX_PYRAMID_GEOM_H
#define DSX_PYRAMID_GEOM_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIP__) || defined(__CUDACC__)
#define DSX_PHD __host__ __device__
#else
#define DSX_PHD
#endif

namespace dsx {
namespace pyr {

constexpr int kMaxLevels = 16;  // level 0 included

// One level's share of a block and where it goes: brick order [rows][nby][nbx][cz][cy][cx], plane 0 of the block's
// level at plane z0 of the brick grid.
struct Level {
  uint16_t* bricks;
  int Z, H, W;     // extent of this level of the block
  int cz, cy, cx;  // chunk shape of the level (already clamped to the level's volume)
  int nby, nbx;    // bricks per axis (ceil)
  int z0;
};

DSX_PHD inline int extent(int n, int level) { return level < 31 ? n >> level : 0; }
DSX_PHD inline uint32_t mean8(uint32_t sum_of_8) { return sum_of_8 >> 3; }  // float64 mean, astype(uint16): floor

// Window of one level step per axis.
struct Scale {
  int fz, fy, fx;
};
DSX_PHD inline bool scale_ok(const Scale& f) {
  return (f.fz == 1 || f.fz == 2) && (f.fy == 1 || f.fy == 2) && (f.fx == 1 || f.fx == 2) && f.fz * f.fy * f.fx > 1;
}
DSX_PHD inline bool scale_is_2(const Scale& f) { return f.fz == 2 && f.fy == 2 && f.fx == 2; }
DSX_PHD inline int extent(int n, int level, int f) { return f == 2 ? extent(n, level) : n; }
DSX_PHD inline int mean_shift(int fz, int fy, int fx) { return (fz - 1) + (fy - 1) + (fx - 1); }  // log2 of the window
DSX_PHD inline uint32_t window_mean(uint32_t sum, int shift) { return sum >> shift; }  // floor, as mean8

// Voxel (z, y, x) of a dense [..][Y][X] stack / of a BrickSrc (below): what window_sum reads through.
struct DenseAt {
  const uint16_t* p;
  size_t slab, row;
  DSX_PHD uint32_t operator()(int z, int y, int x) const { return p[(size_t)z * slab + (size_t)y * row + x]; }
};
// Sum of the fz x fy x fx window of output voxel (z, y, x) in the previous level.
template <class At>
DSX_PHD inline uint32_t window_sum(const At& at, int z, int y, int x, int fz, int fy, int fx) {
  uint32_t s = 0;
  for (int dz = 0; dz < fz; ++dz)
    for (int dy = 0; dy < fy; ++dy)
      for (int dx = 0; dx < fx; ++dx) s += at(fz * z + dz, fy * y + dy, fx * x + dx);
  return s;
}

DSX_PHD inline size_t brick_offset(const Level& g, int z, int y, int x) {
  const int bz = z / g.cz, iz = z - bz * g.cz;
  const int by = y / g.cy, iy = y - by * g.cy;
  const int bx = x / g.cx, ix = x - bx * g.cx;
  const size_t brick = ((size_t)bz * g.nby + by) * g.nbx + bx;
  return ((brick * g.cz + iz) * g.cy + iy) * (size_t)g.cx + ix;
}

// A block that is still in the chunk order it was stored in: [nbz][nby][nbx][cz][cy][cx], every brick full-sized, plane
// 0 of the block at plane 0 of the brick grid (the block starts on a source chunk boundary).  Bricks that stick out of
// the block hold whatever the store held there: positions outside [Z, H, W] are never read.
struct BrickSrc {
  const uint16_t* bricks;
  int cz, cy, cx;  // chunk shape of the source array
  int nby, nbx;    // bricks per axis (ceil)
};

// The offset of voxel (z, y, x) inside a BrickSrc is the sum of a plane, a row and a column part, so a kernel thread
// splits each of its planes, rows and columns once: src_offset below, and k_pyramid_bricks (dsx_pyramid.h).
DSX_PHD inline size_t src_plane(const BrickSrc& s, int z) {
  const int bz = z / s.cz, iz = z - bz * s.cz;
  return ((size_t)bz * s.nby * s.nbx * s.cz + iz) * s.cy * (size_t)s.cx;
}
DSX_PHD inline size_t src_row(const BrickSrc& s, int y) {
  const int by = y / s.cy, iy = y - by * s.cy;
  return ((size_t)by * s.nbx * s.cz * s.cy + iy) * (size_t)s.cx;
}
DSX_PHD inline size_t src_col(const BrickSrc& s, int x) {
  const int bx = x / s.cx, ix = x - bx * s.cx;
  return (size_t)bx * s.cz * s.cy * s.cx + ix;
}
DSX_PHD inline size_t src_offset(const BrickSrc& s, int z, int y, int x) {
  return src_plane(s, z) + src_row(s, y) + src_col(s, x);
}

struct BrickAt {
  BrickSrc s;
  DSX_PHD uint32_t operator()(int z, int y, int x) const { return s.bricks[src_offset(s, z, y, x)]; }
};

inline size_t row_elems(const Level& g) { return (size_t)g.nby * g.nbx * g.cz * g.cy * g.cx; }

// Dense levels 2 .. n_levels - 2 of a block (what the levels >= 3 are computed from), each padded to 16 bytes.
inline size_t work_bytes(int Z, int H, int W, int n_levels) {
  size_t total = 0;
  for (int l = 2; l <= n_levels - 2; ++l) {
    const size_t n = (size_t)extent(Z, l) * extent(H, l) * extent(W, l) * sizeof(uint16_t);
    total += (n + 15) & ~(size_t)15;
  }
  return total;
}
// With a Scale other than (2, 2, 2) every level is one step from the dense previous one: levels 1 .. n_levels - 2.
inline size_t work_bytes(int Z, int H, int W, int n_levels, const Scale& f) {
  if (scale_is_2(f)) return work_bytes(Z, H, W, n_levels);
  size_t total = 0;
  for (int l = 1; l <= n_levels - 2; ++l) {
    const size_t n = (size_t)extent(Z, l, f.fz) * extent(H, l, f.fy) * extent(W, l, f.fx) * sizeof(uint16_t);
    total += (n + 15) & ~(size_t)15;
  }
  return total;
}

// The host build: level by level, every level dense first, then scattered into its bricks.
inline void pyramid_block_host(const uint16_t* planes, int H, int W, int n_levels, const Level* levels,
                               const Scale& f = Scale{2, 2, 2}) {
  std::vector<uint16_t> prev, next;
  DenseAt src = {planes, (size_t)H * W, (size_t)W};
  const int shift = mean_shift(f.fz, f.fy, f.fx);
  for (int l = 1; l < n_levels; ++l) {
    const Level& g = levels[l - 1];
    if (g.Z <= 0 || g.H <= 0 || g.W <= 0) break;
    next.assign((size_t)g.Z * g.H * g.W, 0);
    for (int z = 0; z < g.Z; ++z)
      for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x) {
          const uint16_t v = (uint16_t)window_mean(window_sum(src, z, y, x, f.fz, f.fy, f.fx), shift);
          next[((size_t)z * g.H + y) * g.W + x] = v;
          g.bricks[brick_offset(g, g.z0 + z, y, x)] = v;
        }
    prev.swap(next);
    src = DenseAt{prev.data(), (size_t)g.H * g.W, (size_t)g.W};
  }
}

// The host build from a block in chunk order: the voxels inside [Z, H, W] gathered dense, then the build above.
inline void pyramid_bricks_host(const BrickSrc& s, int Z, int H, int W, int n_levels, const Level* levels,
                                const Scale& f = Scale{2, 2, 2}) {
  std::vector<uint16_t> planes((size_t)Z * H * W);
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < H; ++y) {
      const size_t zy = src_plane(s, z) + src_row(s, y);
      uint16_t* d = planes.data() + ((size_t)z * H + y) * W;
      for (int x = 0; x < W; ++x) d[x] = s.bricks[zy + src_col(s, x)];
    }
  pyramid_block_host(planes.data(), H, W, n_levels, levels, f);
}

}  // namespace pyr
}  // namespace dsx

#endif  // DSX_PYRAMID_GEOM_H
