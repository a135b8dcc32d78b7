// Host build of the pyramid with a scale factor of 1 or 2 per axis (csrc/dsx_pyramid_geom.h: what
// dsx_pyramid_block_scale_ref / dsx_pyramid_bricks_scale_ref run), for tests/test_pyramid_scale_host.py:
//   pyramid_scale_check <block.raw> <Z> <H> <W> <fz> <fy> <fx> <n_levels> <cz> <cy> <cx> <z0> <src_cz> <src_cy> <src_cx>
//                       <result.out>
// reads a dense uint16 block [Z, H, W] and writes, for every level 1 .. n_levels - 1 with a non-empty share, the level's
// bricks [rows][nby][nbx][cz][cy'][cx'] with cy' = min(cy, level rows), cx' = min(cx, level columns), the share at plane
// z0 and rows = ceil((z0 + level planes) / cz).  src_cz > 0: the block is first laid out in chunk order
// [nbz][nby][nbx][src_cz][src_cy][src_cx] and the levels come from pyramid_bricks_host.  The block, the source bricks
// and every level live in heap buffers of exactly their own size, so a sanitizer build sees a window that leaves the
// block, a read of brick padding past the buffer or a store outside a level's rows.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_pyramid_geom.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 17) {
    fprintf(stderr, "usage: %s block.raw Z H W fz fy fx n_levels cz cy cx z0 src_cz src_cy src_cx result.out\n", argv[0]);
    return 1;
  }
  using namespace dsx::pyr;
  int v[14];
  for (int i = 0; i < 14; ++i) v[i] = atoi(argv[2 + i]);
  const int Z = v[0], H = v[1], W = v[2], n_levels = v[6], cz = v[7], cy = v[8], cx = v[9], z0 = v[10];
  const Scale f = {v[3], v[4], v[5]};
  const int scz = v[11], scy = v[12], scx = v[13];
  if (Z < 1 || H < 1 || W < 1 || !scale_ok(f) || n_levels < 1 || n_levels > kMaxLevels || cz < 1 || cy < 1 || cx < 1 || z0 < 0)
    return 1;
  const size_t n = (size_t)Z * H * W;
  std::unique_ptr<uint16_t[]> block(new uint16_t[n]);
  FILE* in = fopen(argv[1], "rb");
  if (!in || fread(block.get(), 2, n, in) != n) return 2;
  fclose(in);

  Level levels[kMaxLevels] = {};
  std::vector<std::unique_ptr<uint16_t[]>> bricks;
  std::vector<size_t> sizes;
  int n_out = 0;
  for (int l = 1; l < n_levels; ++l) {
    Level& g = levels[l - 1];
    g.Z = extent(Z, l, f.fz); g.H = extent(H, l, f.fy); g.W = extent(W, l, f.fx);
    if (g.Z <= 0 || g.H <= 0 || g.W <= 0) break;
    g.cz = cz; g.cy = cy < g.H ? cy : g.H; g.cx = cx < g.W ? cx : g.W;
    g.nby = (g.H + g.cy - 1) / g.cy; g.nbx = (g.W + g.cx - 1) / g.cx;
    g.z0 = z0;
    const size_t elems = (size_t)((z0 + g.Z + cz - 1) / cz) * row_elems(g);
    bricks.emplace_back(new uint16_t[elems]());
    sizes.push_back(elems);
    g.bricks = bricks.back().get();
    n_out = l;
  }
  if (scz > 0) {
    if (scy < 1 || scx < 1) return 1;
    BrickSrc s = {};
    s.cz = scz; s.cy = scy; s.cx = scx;
    s.nby = (H + scy - 1) / scy; s.nbx = (W + scx - 1) / scx;
    const size_t src_elems = (size_t)((Z + scz - 1) / scz) * s.nby * s.nbx * scz * scy * scx;
    std::unique_ptr<uint16_t[]> src(new uint16_t[src_elems]);
    for (size_t i = 0; i < src_elems; ++i) src[i] = 0xFFFF;  // padding: never read
    for (int z = 0; z < Z; ++z)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) src[src_offset(s, z, y, x)] = block[((size_t)z * H + y) * W + x];
    s.bricks = src.get();
    pyramid_bricks_host(s, Z, H, W, n_out + 1, levels, f);
  } else {
    pyramid_block_host(block.get(), H, W, n_out + 1, levels, f);
  }
  FILE* o = fopen(argv[16], "wb");
  if (!o) return 3;
  for (int l = 0; l < n_out; ++l)
    if (fwrite(bricks[l].get(), 2, sizes[l], o) != sizes[l]) return 3;
  fclose(o);
  return 0;
}
