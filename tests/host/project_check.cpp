// Host build of the projections (csrc/dsx_project.h: what dsx_project_u16_ref runs), for tests/test_projections_host.py:
//   project_check <voxels.raw> <first plane> <planes> <H> <W> <out.raw>
// projects `planes` planes of H x W uint16 voxels of <voxels.raw> from plane `first` on, in two calls (the first plane
// alone, then the rest at z_off 1) and writes max_z, sum_z, max_y, sum_y, max_x, sum_x back to back.  The planes are
// copied into a heap buffer of exactly their own size and every array has exactly its own size, so a sanitizer build
// sees a read or a write outside either.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_project.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s voxels.raw first planes H W out.raw\n", argv[0]);
    return 1;
  }
  const size_t first = strtoull(argv[2], nullptr, 10);
  const int Z = atoi(argv[3]), H = atoi(argv[4]), W = atoi(argv[5]);
  const size_t plane = (size_t)H * W, count = (size_t)Z * plane;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint16_t> vox(count);
  if (fseek(f, (long)(first * plane * 2), SEEK_SET) != 0 || fread(vox.data(), 2, count, f) != count) return 2;
  fclose(f);
  std::vector<uint16_t> max_z(plane, 0xABCD), max_y((size_t)Z * W, 0xABCD), max_x((size_t)Z * H, 0xABCD);
  std::vector<uint64_t> sum_z(plane, 77);
  std::vector<uint32_t> sum_y((size_t)Z * W, 77), sum_x((size_t)Z * H, 77);
  const dsx::pj::Outputs o = {max_z.data(), sum_z.data(), max_y.data(), sum_y.data(), max_x.data(), sum_x.data()};
  dsx::pj::project_host(vox.data(), Z > 0 ? 1 : 0, H, W, o, 0, true);  // `first` overwrites what the z arrays held
  if (Z > 1) dsx::pj::project_host(vox.data() + plane, Z - 1, H, W, o, 1, false);
  dsx::pj::project_host(vox.data(), 0, H, W, o, 0, false);  // no planes: nothing changes
  FILE* out = fopen(argv[6], "wb");
  if (!out) return 3;
  bool ok = fwrite(max_z.data(), 2, max_z.size(), out) == max_z.size();
  ok = ok && fwrite(sum_z.data(), 8, sum_z.size(), out) == sum_z.size();
  ok = ok && fwrite(max_y.data(), 2, max_y.size(), out) == max_y.size();
  ok = ok && fwrite(sum_y.data(), 4, sum_y.size(), out) == sum_y.size();
  ok = ok && fwrite(max_x.data(), 2, max_x.size(), out) == max_x.size();
  ok = ok && fwrite(sum_x.data(), 4, sum_x.size(), out) == sum_x.size();
  fclose(out);
  return ok ? 0 : 3;
}
