// Host build of the zstd frame decoder of the device path (csrc/dsx_zstd_dec.h), for tests/test_zstd_decoder_host.py:
//   zstd_dec_check decode <records> <out>          decode every record; <out>: per record int32 status + the bytes
//   zstd_dec_check mutate <records> <iters> <seed> every truncation of every record, then <iters> seeded bit flips and
//                                                  byte overwrites each; prints "<status> <count>" per outcome
// <records>: back to back [uint32 frame bytes][uint32 output bytes][frame].  The inputs live in buffers of exactly
// their size, so a sanitizer build sees any read past a frame.  A mutated frame must end in an error status or in
// exactly the expected number of bytes.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_zstd_dec.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

namespace z = dsx::zdec;

static bool load(const char* path, std::vector<std::pair<std::vector<uint8_t>, uint32_t>>& recs) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (;;) {
    uint32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) break;
    std::vector<uint8_t> fr(hdr[0]);
    if (hdr[0] && fread(fr.data(), 1, hdr[0], f) != hdr[0]) { fclose(f); return false; }
    recs.emplace_back(std::move(fr), hdr[1]);
  }
  fclose(f);
  return true;
}

static int run(z::Tables& t, const std::vector<uint8_t>& fr, uint32_t want, std::vector<uint8_t>& out) {
  // exact-size copies: a read one byte past the frame or a write one byte past the output is a sanitizer report
  uint8_t* in = new uint8_t[fr.size() ? fr.size() : 1];
  if (!fr.empty()) memcpy(in, fr.data(), fr.size());
  uint8_t* o = new uint8_t[want ? want : 1];
  const int st = z::decode_frame(t, in, (uint32_t)fr.size(), o, want);
  out.assign(o, o + want);
  delete[] o;
  delete[] in;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s decode|mutate records ...\n", argv[0]); return 2; }
  std::vector<std::pair<std::vector<uint8_t>, uint32_t>> recs;
  if (!load(argv[2], recs)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  z::Tables* t = new z::Tables;
  std::vector<uint8_t> out;
  if (!strcmp(argv[1], "decode")) {
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    for (auto& r : recs) {
      const int32_t st = run(*t, r.first, r.second, out);
      fwrite(&st, 4, 1, o);
      if (st == 0 && r.second) fwrite(out.data(), 1, r.second, o);
    }
    fclose(o);
    delete t;
    return 0;
  }
  if (strcmp(argv[1], "mutate") || argc < 5) return 2;
  const int iters = atoi(argv[3]);
  std::mt19937 rng((unsigned)atoi(argv[4]));
  std::map<int, int> seen;
  for (auto& r : recs) {
    for (size_t cut = 0; cut < r.first.size(); ++cut) {
      std::vector<uint8_t> f(r.first.begin(), r.first.begin() + cut);
      seen[run(*t, f, r.second, out)]++;
    }
    for (int it = 0; it < iters && !r.first.empty(); ++it) {
      std::vector<uint8_t> f = r.first;
      const int k = 1 + (int)(rng() % 4);
      for (int j = 0; j < k; ++j) {
        const size_t p = rng() % f.size();
        if (rng() & 1) f[p] ^= (uint8_t)(1u << (rng() % 8));
        else f[p] = (uint8_t)rng();
      }
      seen[run(*t, f, r.second, out)]++;
    }
  }
  for (auto& kv : seen) printf("%d %d\n", kv.first, kv.second);
  delete t;
  return 0;
}
