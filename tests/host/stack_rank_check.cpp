// Host build of the stack-rank kernel's contract (csrc/dsx_stackrank.h: what dsx_stack_rank_u16_ref runs), for
// tests/test_stack_rank_host.py:
//   stack_rank_check <stack.raw> <lead> <n> <P> <lo> <hi> <n_q> <q0> .. <q3> <result.out>
// reads n * P uint16 from element `lead` of <stack.raw> on and writes out [n_q][P] followed by valid [P].  The stack and
// the results live in heap buffers of exactly their own size, so a sanitizer build sees a read or a write outside them.
// It also walks the launch geometry over every n: the tile fits 64 KiB, TP * S = 256, the tiles cover P exactly.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_stackrank.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  namespace sr = dsx::sr;
  if (argc != 13) {
    fprintf(stderr, "usage: %s stack.raw lead n P lo hi n_q q0 q1 q2 q3 result.out\n", argv[0]);
    return 1;
  }
  const size_t lead = strtoull(argv[2], nullptr, 10);
  const int n = atoi(argv[3]);
  const size_t P = strtoull(argv[4], nullptr, 10);
  const int lo = atoi(argv[5]), hi = atoi(argv[6]), n_q = atoi(argv[7]);
  const int q[4] = {atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), atoi(argv[11])};

  for (int k = 1; k <= sr::kSrMaxPlanes; ++k) {
    const sr::Geometry g = sr::geometry(k, P);
    if (g.tile_bytes > sr::kSrTileLimit || g.tp * g.slices != sr::kSrThreads) return 4;
    if (g.grid * (size_t)g.tp < P || (g.grid - 1) * (size_t)g.tp >= P) return 4;
  }

  std::vector<uint16_t> stack((size_t)n * P), out((size_t)n_q * P), valid(P);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  if (fseek(f, (long)(lead * 2), SEEK_SET) != 0 || fread(stack.data(), 2, stack.size(), f) != stack.size()) return 2;
  fclose(f);
  if (sr::check_args(stack.data(), n, P, lo, hi, q, n_q, out.data())) return 5;
  sr::stack_rank_host(stack.data(), n, P, lo, hi, q, n_q, out.data(), nullptr);  // valid may be NULL
  sr::stack_rank_host(stack.data(), n, P, lo, hi, q, n_q, out.data(), valid.data());
  FILE* o = fopen(argv[12], "wb");
  if (!o || fwrite(out.data(), 2, out.size(), o) != out.size() || fwrite(valid.data(), 2, P, o) != P) return 3;
  fclose(o);
  return 0;
}
