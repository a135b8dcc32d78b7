// Host build of the chunk digest's contract (csrc/dsx_digest.h: what dsx_brick_digest_u16_ref runs), for
// tests/test_digest_host.py:
//   digest_check <bricks.raw> <lead> n0 n1 n2 c0 c1 c2 v0 v1 v2 <records.out>
// reads n0 * n1 * n2 bricks of c0 * c1 * c2 uint16 from element `lead` of <bricks.raw> on and writes the records,
// uint64 [bricks][3].  The bricks and the records live in heap buffers of exactly their own size, so a sanitizer build
// sees a read or a write outside them.  It also checks the known answers of the weight and walks the launch geometry
// over row lengths and brick heights: lanes along a row a power of two that covers the row's vectors (up to the block),
// lx * ly = the block, segments that cover the rows exactly, and the refusals of check_geometry.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_digest.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  namespace dg = dsx::dg;
  if (argc != 13) {
    fprintf(stderr, "usage: %s bricks.raw lead n0 n1 n2 c0 c1 c2 v0 v1 v2 records.out\n", argv[0]);
    return 1;
  }
  if (dg::weight(0) != 0xe220a8397b1dcdafull || dg::weight(1) != 0x6e789e6aa1b965f5ull ||
      dg::weight(1ull << 32) != 0x46093cf9861ec2e5ull)
    return 6;
  if (dg::extent(5, 9, 1) != 4 || dg::extent(5, 10, 1) != 5 || dg::extent(5, 9, 0) != 5) return 6;

  for (int c2 = 1; c2 <= 5000; ++c2)
    for (int rows : {1, 2, 511, 512, 513, 8192}) {
      const dg::Geometry g = dg::geometry(3, rows, 1, c2);
      const int nvec = (c2 + 7) / 8;
      if (g.lx * g.ly != dg::kDgThreads || (g.lx & (g.lx - 1))) return 4;
      if (g.lx < nvec && g.lx != dg::kDgThreads) return 4;
      if (g.lx > 1 && g.lx / 2 >= nvec) return 4;
      if (g.segs * dg::kDgSegRows < rows || (g.segs - 1) * dg::kDgSegRows >= rows || g.grid != 3 * g.segs) return 4;
    }
  if (dg::check_geometry(1, 1, 1, 1, 1, 1, 1, 1, 1)) return 5;
  if (dg::check_geometry(1, 1, 1, 1 << 10, 1 << 10, 1 << 11, 1, 1, 1)) return 5;            // 2^31 voxels: taken
  if (!dg::check_geometry(1, 1, 1, 1 << 10, 1 << 10, (1 << 11) + 1, 1, 1, 1)) return 5;     // one row more: refused
  if (!dg::check_geometry(1, 1, 1, 1 << 16, 1 << 16, 1, 1, 1, 1)) return 5;
  if (!dg::check_geometry(0, 1, 1, 2, 2, 2, 1, 1, 1) || !dg::check_geometry(1, 1, 1, 2, 0, 2, 1, 1, 1)) return 5;
  if (!dg::check_geometry(2, 1, 1, 4, 4, 4, 4, 4, 4)) return 5;   // the second brick would be empty
  if (!dg::check_geometry(2, 1, 1, 4, 4, 4, 9, 4, 4)) return 5;   // voxels outside the grid
  if (!dg::check_geometry(1, 1, 1, 4, 4, 4, 4, 0, 4)) return 5;

  const size_t lead = strtoull(argv[2], nullptr, 10);
  int a[9];
  for (int k = 0; k < 9; ++k) a[k] = atoi(argv[3 + k]);
  if (dg::check_geometry(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8])) return 5;
  const size_t bricks = (size_t)a[0] * a[1] * a[2], brick = (size_t)a[3] * a[4] * a[5];
  std::vector<uint16_t> vox(bricks * brick);
  std::vector<uint64_t> out(bricks * dg::kDgRecord);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  if (fseek(f, (long)(lead * 2), SEEK_SET) != 0 || fread(vox.data(), 2, vox.size(), f) != vox.size()) return 2;
  fclose(f);
  dg::grid_digest_host(vox.data(), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], out.data());
  FILE* o = fopen(argv[12], "wb");
  if (!o || fwrite(out.data(), 8, out.size(), o) != out.size()) return 3;
  fclose(o);
  return 0;
}
