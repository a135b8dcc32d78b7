// Host build of the zstd frame decoder of the device path (csrc/dsx_zstd_dec.h; the watermark rule of
// csrc/dsx_zdec_task.h), for tests/test_zstd_decoder_host.py:
//   zstd_dec_check decode <records> <out>          decode every record; <out>: per record int32 status + the bytes
//   zstd_dec_check mutate <records> <iters> <seed> every truncation of every record, then <iters> seeded bit flips and
//                                                  byte overwrites each; prints "<status> <count>" per outcome
//   zstd_dec_check stats <records> <batch>         walk every record with the shared seq_header / next_seq and print one
//                                                  line of counts per record (kStatNames, after a line of the names):
//                                                  what the frame asks of the device driver, whose sequence batches hold
//                                                  <batch> sequences (the watermark of dsx_zdec_kernels.h is replayed)
// <records>: back to back [uint32 frame bytes][uint32 output bytes][frame].  The inputs live in buffers of exactly
// their size, so a sanitizer build sees any read past a frame.  A mutated frame must end in an error status or in
// exactly the expected number of bytes.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_zdec_task.h"

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

// ---- stats: the cases of one frame that only the sequences show -------------------------------------------------------
enum Stat {
  kStatus, kBlocks, kRawBlocks, kRleBlocks, kCompBlocks, kMaxSeq, kMaxStream, kHuf1, kHuf4, kTreelessLater, kSeqs,
  kOffGeMl, kPatDiv, kPatNoDiv, kOff1, kBarOwnLit, kBarPrevMatch, kBarriers, kMaxFreeRun, kRepeat, kStats
};
static const char* kStatNames =
    "status blocks raw_blocks rle_blocks comp_blocks max_seq max_stream huf1 huf4 treeless_later seqs off_ge_ml pat_div "
    "pat_nodiv off1 bar_own_lit bar_prev_match barriers max_free_run repeat";

// The blocks of a frame as decode_frame takes them, without an output: the literals are only measured, the sequences
// are decoded and validated by next_seq.  `fenced` is the watermark of zstd_wave: output below it is visible to the
// wave, a match whose source reaches above it (match_needs_fence of csrc/dsx_zdec_task.h, which the kernel runs)
// passes a barrier first; the end of a batch of `batch` sequences is one.
static void walk(z::Tables& t, const uint8_t* s, uint32_t n, uint32_t out_n, uint32_t batch, long* c) {
  for (int i = 0; i < kStats; ++i) c[i] = 0;
  z::FrameHdr fh;
  int st = z::frame_header(s, n, fh);
  if (st) { c[kStatus] = st; return; }
  t.huf_log = 0;
  t.ll_log = t.of_log = t.ml_log = -1;
  z::SeqState q;
  q.rep0 = 1; q.rep1 = 4; q.rep2 = 8;
  uint32_t ip = fh.bytes, op = 0;
  for (;;) {
    if (n - ip < 3) { c[kStatus] = z::kErrTruncated; return; }
    const uint32_t bh = z::le(s + ip, 3);
    ip += 3;
    const int last = (int)(bh & 1), type = (int)((bh >> 1) & 3);
    const uint32_t bs = bh >> 3;
    if (type == 3 || bs > z::kBlockMax || (type != 1 && bs > n - ip) || (type == 1 && n - ip < 1)) {
      c[kStatus] = z::kErrTruncated;
      return;
    }
    c[kBlocks]++;
    if (type < 2) {
      if (bs > out_n - op) { c[kStatus] = z::kErrOutput; return; }
      c[type == 0 ? kRawBlocks : kRleBlocks]++;
      ip += type == 0 ? bs : 1;
      op += bs;
    } else {
      c[kCompBlocks]++;
      const uint8_t* b = s + ip;
      z::LitHdr lh;
      st = z::lit_header(b, bs, lh);
      if (!st && lh.regen > out_n - op) st = z::kErrOutput;
      if (st) { c[kStatus] = st; return; }
      if (lh.type >= 2) {
        uint32_t tree = 0;
        if (lh.type == 2) {
          const int used = z::read_huf_tree(t, b + lh.hdr, lh.csize);
          if (used < 0) { c[kStatus] = -used; return; }
          tree = (uint32_t)used;
        } else if (c[kBlocks] > 1) {
          c[kTreelessLater]++;
        }
        z::Streams ss;
        st = z::split_streams(b + lh.hdr + tree, lh.csize - tree, lh.regen, lh.streams, ss);
        if (st) { c[kStatus] = st; return; }
        c[lh.streams == 1 ? kHuf1 : kHuf4]++;
        for (int k = 0; k < lh.streams; ++k)
          if ((long)ss.len[k] > c[kMaxStream]) c[kMaxStream] = (long)ss.len[k];
      }
      const uint32_t sp = lh.hdr + lh.csize;
      uint32_t nseq = 0;
      q.op = op;
      q.lit_used = 0;
      q.nlit = lh.regen;
      st = z::seq_header(t, b + sp, bs - sp, q, &nseq);
      if (st) { c[kStatus] = st; return; }
      if ((long)nseq > c[kMaxSeq]) c[kMaxSeq] = (long)nseq;
      uint32_t wop = op, fenced = op, prev_match = 0;
      long run = 0;
      for (uint32_t k = 0; k < nseq; ++k) {
        if (k && k % batch == 0) {  // the barrier that ends a batch
          fenced = wop;
          run = 0;
        }
        const int ofc = t.of[q.sof].sym;
        z::Seq e;
        st = z::next_seq(t, q, out_n, e);
        if (st) { c[kStatus] = st; return; }
        c[kSeqs]++;
        if (ofc <= 1) c[kRepeat]++;  // offset values 1 .. 3: the repeat offsets
        wop += e.ll;
        const uint32_t src = wop - e.off, span = e.ml < e.off ? e.ml : e.off;  // (the bytes the match loads)
        if (e.off >= e.ml) c[kOffGeMl]++;
        else c[64u % e.off == 0 ? kPatDiv : kPatNoDiv]++;
        if (e.off == 1) c[kOff1]++;
        if (z::match_needs_fence(src, e.ml, e.off, fenced)) {  // the rule wave_match runs
          c[kBarriers]++;
          const bool own = e.ll > 0 && src + span > wop - e.ll;  // the source holds literals of this sequence
          if (own) c[kBarOwnLit]++;
          else if (k % batch != 0 && src + span > prev_match) c[kBarPrevMatch]++;  // ... bytes of the match before it
          fenced = wop;
          run = 0;
        } else if (++run > c[kMaxFreeRun]) {
          c[kMaxFreeRun] = run;
        }
        prev_match = wop;
        wop += e.ml;
      }
      if (nseq && (st = z::seq_end(q))) { c[kStatus] = st; return; }
      const uint32_t rest = lh.regen - q.lit_used;
      if (rest > out_n - q.op) { c[kStatus] = z::kErrOutput; return; }
      op = q.op + rest;
      ip += bs;
    }
    if (last) break;
  }
  if (op != out_n) c[kStatus] = z::kErrOutput;
  else if (ip != n) c[kStatus] = z::kErrTruncated;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s decode|mutate|stats records ...\n", argv[0]); return 2; }
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
  if (!strcmp(argv[1], "stats")) {
    const int batch = atoi(argv[3]);
    if (batch < 1) return 2;
    printf("%s\n", kStatNames);
    for (auto& r : recs) {
      long c[kStats];
      walk(*t, r.first.data(), (uint32_t)r.first.size(), r.second, (uint32_t)batch, c);
      for (int i = 0; i < kStats; ++i) printf(i + 1 < kStats ? "%ld " : "%ld\n", c[i]);
    }
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
