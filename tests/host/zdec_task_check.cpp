// Host build of the Blosc block tasks of the device path (csrc/dsx_zdec_task.h: run_task_host over every kind and
// flag), for the host tests of the decoders (tests/zdec_cases.py build_check_exe):
//   zdec_task_check decode <records> <out>          run every record; <out>: per record int32 status + the bytes
//   zdec_task_check mutate <records> <iters> <seed> every truncation of every record, then <iters> seeded single-byte
//                                                   mutations each; prints "<status> <same bytes> <count>" per
//                                                   outcome (same bytes: 1 when status 0 came with the original output)
// <records>: back to back [uint32 task bytes][uint32 output bytes][uint32 kind][task bytes]: one DecTask whose src is
// the whole record.  The inputs live in buffers of exactly their size, so a sanitizer build sees any read past the
// task's bytes and any write past its output.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_zdec_task.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

namespace z = dsx::zdec;

struct Rec {
  std::vector<uint8_t> bytes;
  uint32_t want, kind;
};

static bool load(const char* path, std::vector<Rec>& recs) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (;;) {
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) break;
    Rec r;
    r.bytes.resize(hdr[0]);
    r.want = hdr[1];
    r.kind = hdr[2];
    if (hdr[0] && fread(r.bytes.data(), 1, hdr[0], f) != hdr[0]) { fclose(f); return false; }
    recs.push_back(std::move(r));
  }
  fclose(f);
  return true;
}

static int run(z::DecWork& t, const std::vector<uint8_t>& in_, uint32_t want, uint32_t kind, std::vector<uint8_t>& out) {
  uint8_t* in = new uint8_t[in_.size() ? in_.size() : 1];
  if (!in_.empty()) memcpy(in, in_.data(), in_.size());
  uint8_t* o = new uint8_t[want ? want : 1];
  uint8_t* tmp = new uint8_t[want ? want : 1];
  memset(o, 0, want ? want : 1);
  const z::DecTask k{0, 0, (uint32_t)in_.size(), want, kind, 0};
  const int st = z::run_task_host(t, k, in, o, tmp);
  out.assign(o, o + want);
  delete[] tmp;
  delete[] o;
  delete[] in;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s decode|mutate records ...\n", argv[0]); return 2; }
  std::vector<Rec> recs;
  if (!load(argv[2], recs)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  z::DecWork* t = new z::DecWork;
  std::vector<uint8_t> out;
  if (!strcmp(argv[1], "decode")) {
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    for (auto& r : recs) {
      const int32_t st = run(*t, r.bytes, r.want, r.kind, out);
      fwrite(&st, 4, 1, o);
      if (st == 0 && r.want) fwrite(out.data(), 1, r.want, o);
    }
    fclose(o);
    delete t;
    return 0;
  }
  if (strcmp(argv[1], "mutate") || argc < 5) return 2;
  const int iters = atoi(argv[3]);
  std::mt19937 rng((unsigned)atoi(argv[4]));
  std::map<std::pair<int, int>, int> seen;
  for (auto& r : recs) {
    std::vector<uint8_t> good;
    if (run(*t, r.bytes, r.want, r.kind, good) != 0) { fprintf(stderr, "a record does not decode\n"); return 3; }
    auto one = [&](const std::vector<uint8_t>& f) {
      const int st = run(*t, f, r.want, r.kind, out);
      seen[{st, st == 0 && out == good ? 1 : 0}]++;
    };
    for (size_t cut = 0; cut < r.bytes.size(); ++cut) one(std::vector<uint8_t>(r.bytes.begin(), r.bytes.begin() + cut));
    for (int it = 0; it < iters && !r.bytes.empty(); ++it) {
      std::vector<uint8_t> f = r.bytes;
      const size_t p = rng() % f.size();  // one byte: a bit flip, or another value
      if (rng() & 1) f[p] ^= (uint8_t)(1u << (rng() % 8));
      else f[p] = (uint8_t)(f[p] + 1 + rng() % 255);
      one(f);
    }
  }
  for (auto& kv : seen) printf("%d %d %d\n", kv.first.first, kv.first.second, kv.second);
  delete t;
  return 0;
}
