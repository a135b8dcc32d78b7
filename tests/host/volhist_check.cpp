// Host build of the voxel histogram (csrc/dsx_volhist.h: what dsx_volhist_ref runs), for tests/test_volhist_host.py:
//   volhist_check <voxels.raw> <first voxel> <count> <hist.out>
// counts `count` uint16 voxels of <voxels.raw> from voxel `first` on and writes the 65 536 uint64 bins.  The range is
// copied into a heap buffer of exactly its own size and the bins are exactly 65 536 words, so a sanitizer build sees a
// read or a count outside either.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_volhist.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s voxels.raw first count hist.out\n", argv[0]);
    return 1;
  }
  const size_t first = strtoull(argv[2], nullptr, 10), count = strtoull(argv[3], nullptr, 10);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint16_t> vox(count);
  if (fseek(f, (long)(first * 2), SEEK_SET) != 0 || fread(vox.data(), 2, count, f) != count) return 2;
  fclose(f);
  std::vector<uint64_t> hist(dsx::vh::kVhBins, 0);
  dsx::vh::volhist_host(vox.data(), count, hist.data());
  dsx::vh::volhist_host(vox.data(), 0, hist.data());  // n == 0 adds nothing
  FILE* o = fopen(argv[4], "wb");
  if (!o || fwrite(hist.data(), 8, hist.size(), o) != hist.size()) return 3;
  fclose(o);
  return 0;
}
