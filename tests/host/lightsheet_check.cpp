// Host build of the light-sheet background mode (csrc/dsx_lightsheet.h: what dsx_lightsheet_ref runs), for
// tests/test_lightsheet_host.py:
//   lightsheet_check <plane.raw> <H> <W> <p> <A> <B> <lambda> <tables.raw> <result.out>
// reads a uint16 plane [H, W] and the tables (255 uint32 edges, then 256 float32 values), checks the arguments as the
// entry point does, and writes ls (uint8), bg (uint8) and out (float32), [H, W] each.  The plane, the tables and every
// result live in heap buffers of exactly their own size, so a sanitizer build sees a read past a border or a count
// outside the 256 bins.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_lightsheet.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s plane.raw H W p A B lambda tables.raw result.out\n", argv[0]);
    return 1;
  }
  using namespace dsx::ls;
  const int H = atoi(argv[2]), W = atoi(argv[3]), A = atoi(argv[5]), B = atoi(argv[6]);
  const double p = strtod(argv[4], nullptr), lambda = strtod(argv[7], nullptr);
  if (H < 1 || W < 1) return 1;
  const size_t n = (size_t)H * W;
  std::vector<uint16_t> x(n);
  std::vector<uint32_t> edges(kLsEdges);
  std::vector<float> back(256);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(x.data(), 2, n, f) != n) return 2;
  fclose(f);
  f = fopen(argv[8], "rb");
  if (!f || fread(edges.data(), 4, edges.size(), f) != edges.size() || fread(back.data(), 4, back.size(), f) != back.size())
    return 2;
  fclose(f);
  if (const char* e = lightsheet_args(H, W, p, A, B, lambda, edges.data(), back.data())) {
    fprintf(stderr, "%s\n", e);
    return 4;
  }
  std::vector<uint8_t> q(n), ls(n), bg(n);
  std::vector<float> out(n);
  lightsheet_host(x.data(), H, W, p, A, B, (float)lambda, edges.data(), back.data(), q.data(), ls.data(), bg.data(),
                  out.data());
  FILE* o = fopen(argv[9], "wb");
  if (!o || fwrite(ls.data(), 1, n, o) != n || fwrite(bg.data(), 1, n, o) != n || fwrite(out.data(), 4, n, o) != n) return 3;
  fclose(o);
  return 0;
}
