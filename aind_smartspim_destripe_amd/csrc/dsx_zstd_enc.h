// dsx_zstd_enc.h -- entropy-only zstd inside Blosc frames: the encoder core shared by the host reference and the
// device kernels (dsx_zenc_kernels.h).  Plain C++; g++ builds it for the CPU tests (tests/host/zstd_enc_check.cpp).
//
// Format (RFC 8878): one zstd frame per Blosc block -- magic, single-segment frame header with the content size, no
// checksum -- holding zstd blocks of <= 128 KiB.  A block whose bytes are all equal is an RLE block; otherwise its
// literals are Huffman-coded (4 streams, Size_Format 11, 6-byte jump table, code lengths <= 11 bits, weights
// FSE-compressed with table log 6 and two interleaved states, or in the direct 4-bit form when that is smaller) with a
// sequences section of zero sequences; a block that does not get smaller is stored raw.  No match finder: about
// 1.1-1.2x the bytes of zstd level 5 on byte-shuffled uint16 image bricks.
//
// Runs mode (kModeRuns; the entropy-only mode above stays the default and its bytes are unchanged): a compressed block
// may carry sequences.  Every maximal run of >= kMinRun equal bytes inside a zstd block becomes one literal (its first
// byte) and one match of offset 1 over the rest; a run never crosses a zstd block.  The sequences section uses
// Predefined_Mode for literal lengths, offsets and match lengths (the distributions and the length-code baselines are
// those of dsx_zstd_dec.h), three interleaved FSE states, written back to front by one thread.  Every sequence has a
// literal length >= 1 (the run's first byte) and the repeat offsets of a frame start at (1, 4, 8), so every match is
// Offset_Value 1 = repeat offset 1 = distance 1: the offset history never changes, which keeps the matches valid across
// the blocks of a frame, and no sequence with literal length 0 is ever written.  The remaining literals are one of
// RLE_Literals_Block, Raw_Literals_Block or Huffman (four streams, as above), the smallest, ties in that order.  Per
// zstd block the smaller of this encoding and the entropy-only one is taken, ties to the entropy-only one, so a frame
// is never larger than the entropy-only frame of its chunk.
//   kMinRun = 8: a sequence costs at most 6 + 6 + 5 state bits and 16 + 16 extra bits = 49 bits, less than the 7 bytes
//   the shortest match removes, so the sequences stream always fits behind the compacted literals in a work buffer of
//   one slot; on image bricks the total hardly depends on the threshold (4 ... 32 within 0.1 % in a model of the sizes).
//   kSeqCap = 1024 sequences per block (bricks of image data stay under 400): it bounds the single-thread FSE chain and
//   the sequence list on adversarial input.  The first kSeqCap qualifying runs in position order are kept, later ones
//   stay literals.
// No general matches, no offsets other than 1, no fitted FSE tables.
//
// Blosc container (dsx_blosc_frame.h, ZstdFrames below): what dsx_io.h blosc_encode writes -- version 2, 256 KiB
// blocks, byte shuffle, "don't split", a stream as long as its block = stored; a frame not smaller than its data
// becomes a memcpyed frame.  Typesize 2 only.
//
// Determinism: every choice below (the histogram, the sort key, the code lengths, the weight normalisation) is a
// function of the block's bytes, so the device kernels write exactly the bytes of the host build.
#ifndef DSX_ZSTD_ENC_H
#define DSX_ZSTD_ENC_H

#include <stddef.h>
#include <stdint.h>

#include "dsx_blosc_frame.h"  // the container: Geometry, shuffled_byte, put_le, the slots, assemble_chunks_host
#include "dsx_zstd_dec.h"     // the predefined distributions and the length-code baselines of the sequences

// The single-thread planners below are used by two kernels; left to the inliner they become calls (k_zenc_block then
// takes 88 VGPRs instead of 50).
#define DSX_ZPLAN DSX_ZHD inline __attribute__((always_inline))

namespace dsx {
namespace zenc {

using namespace blosc;

constexpr int kZBlock = 128 * 1024;             // zstd Block_Maximum_Size
constexpr int kMaxBits = 11;                    // Huffman code length limit
constexpr int kMinHuf = 64;                     // shorter blocks: raw or RLE (4 streams need a few literals each)
constexpr int kTreeCap = 160;                   // Huffman tree description: 1 + <= 128 bytes (+ slack for FSE)
constexpr int kFseLog = 6;                      // table log of the weight FSE
enum BlockType { kRaw = 0, kRle = 1, kCompressed = 2 };  // also the literals section types of the runs mode
enum Mode { kModeLiterals = 0, kModeRuns = 1 };
constexpr int kMinRun = 8;                      // runs mode: shortest run that becomes a match
constexpr int kSeqCap = 1024;                   // runs mode: sequences per zstd block at most

// Working state of one zstd block (LDS on the device, ~8 KB).
struct HufWork {
  uint32_t scount[4][256];  // histogram per literal stream
  uint32_t count[256];      // histogram of the block
  uint32_t sorted[256];     // (count << 8 | symbol) of the present symbols, ascending
  uint32_t a[256];          // code-length construction
  uint16_t code[256];
  uint8_t len[256];
  uint8_t wgt[256];
  uint8_t tree[kTreeCap];   // Huffman tree description (header byte + weights)
  uint8_t fse_sym[1 << kFseLog];
  uint16_t fse_state[1 << kFseLog];
  int16_t norm[16];
  uint32_t wc[16];          // (the small tables of the single-thread parts live here too: no private arrays)
  int32_t dnb[16], dfs[16], cumul[17];
  int bl[kMaxBits + 2];
  uint32_t start[kMaxBits + 2];
  uint32_t stream_bytes[4];
  int nsym, type, tree_bytes, block_bytes, max_bits, prefix_bytes;
  uint8_t rle_byte;
};

DSX_ZHD inline int highbit(uint32_t v) {  // v > 0
  int r = 0;
  while (v >>= 1) ++r;
  return r;
}

// little-endian bit writer of the single-thread parts (FSE weights, host streams)
struct BitW {
  uint8_t* out;
  int cap, pos, nb;
  uint64_t acc;
  bool ovf;
  DSX_ZHD BitW(uint8_t* o, int c) : out(o), cap(c), pos(0), nb(0), acc(0), ovf(false) {}
  DSX_ZHD void add(uint32_t v, int n) {
    acc |= (uint64_t)(v & ((n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u))) << nb;
    nb += n;
    while (nb >= 8) {
      if (pos < cap) out[pos] = (uint8_t)acc;
      else ovf = true;
      ++pos;
      acc >>= 8;
      nb -= 8;
    }
  }
  DSX_ZHD int flush() {  // pad to a byte; bytes written, -1 on overflow
    if (nb > 0) add(0, 8 - nb);
    return ovf ? -1 : pos;
  }
  DSX_ZHD int close() {  // end mark + pad (backward-read streams)
    add(1, 1);
    return flush();
  }
};

// literal stream k of a block of n literals covers [stream_begin(k), stream_begin(k + 1))
DSX_ZHD inline int stream_begin(int n, int k) {
  const int seg = (n + 3) / 4;
  return k * seg < n ? k * seg : n;
}

// sort key of symbol s (only symbols with count > 0 take part): rank = keys below it
DSX_ZHD inline uint32_t sort_key(const HufWork& w, int s) { return (w.count[s] << 8) | (uint32_t)s; }
DSX_ZHD inline int sort_rank(const HufWork& w, int s) {
  const uint32_t k = sort_key(w, s);
  int r = 0;
  for (int t = 0; t < 256; ++t) r += (w.count[t] != 0 && sort_key(w, t) < k) ? 1 : 0;
  return r;
}

// Minimum-redundancy code lengths in place (Moffat & Katajainen 1995): a[0 .. n) ascending weights -> lengths
// (a[0] the longest).  n >= 2.
DSX_ZPLAN void mk_lengths(uint32_t* a, int n) {
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < n - 1; ++next) {
    if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = next; }
    else a[next] = a[leaf++];
    if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = next; }
    else a[next] += a[leaf++];
  }
  a[n - 2] = 0;
  for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
  int avbl = 1, used = 0, dpth = 0, root2 = n - 2, next = n - 1;
  while (avbl > 0) {
    while (root2 >= 0 && (int)a[root2] == dpth) { ++used; --root2; }
    while (avbl > used) { a[next--] = dpth; --avbl; }
    avbl = 2 * used;
    ++dpth;
    used = 0;
  }
}

// FSE-compressed Huffman weights w[0 .. nw) -> out (table log 6, two interleaved states, as zstd's
// FSE_compress_usingCTable).  Returns the bytes, or 0 when FSE does not apply / does not fit `cap`.
DSX_ZPLAN int fse_weights(HufWork& h, const uint8_t* w, int nw, uint8_t* out, int cap) {
  constexpr int L = kFseLog, T = 1 << kFseLog;
  uint32_t* wc = h.wc;
  for (int v = 0; v < 16; ++v) wc[v] = 0;
  for (int i = 0; i < nw; ++i) wc[w[i]]++;
  int distinct = 0, maxv = 0;
  for (int v = 0; v < 16; ++v) if (wc[v]) { ++distinct; maxv = v; }
  if (nw <= 2 || distinct < 2) return 0;
  // normalised counts: every present weight >= 1, sum 64
  int16_t* norm = h.norm;
  int sum = 0;
  for (int v = 0; v < 16; ++v) {
    norm[v] = (int16_t)(wc[v] ? (int)(wc[v] * T / (uint32_t)nw) : 0);
    if (wc[v] && norm[v] < 1) norm[v] = 1;
    sum += norm[v];
  }
  while (sum > T) {
    int best = -1;
    for (int v = 0; v < 16; ++v) if (norm[v] > 1 && (best < 0 || norm[v] > norm[best])) best = v;
    norm[best]--;
    --sum;
  }
  if (sum < T) {
    int best = 0;
    for (int v = 1; v < 16; ++v) if (wc[v] > wc[best]) best = v;
    norm[best] = (int16_t)(norm[best] + (T - sum));
  }
  BitW bw(out, cap);
  // table description (FSE_writeNCount)
  bw.add(L - 5, 4);
  {
    int remaining = T + 1, threshold = T, nbBits = L + 1;
    int sym = 0;
    bool prev0 = false;
    while (sym <= maxv && remaining > 1) {
      if (prev0) {
        int start = sym;
        while (sym <= maxv && !norm[sym]) ++sym;
        while (sym >= start + 24) { start += 24; bw.add(0xFFFFu, 16); }
        while (sym >= start + 3) { start += 3; bw.add(3, 2); }
        bw.add((uint32_t)(sym - start), 2);
      }
      int count = norm[sym++];
      const int max = (2 * threshold - 1) - remaining;
      remaining -= count;
      ++count;
      if (count >= threshold) count += max;
      bw.add((uint32_t)count, count < max ? nbBits - 1 : nbBits);
      prev0 = (count == 1);
      while (remaining < threshold) { --nbBits; threshold >>= 1; }
    }
  }
  if (bw.nb > 0) bw.add(0, 8 - bw.nb);  // the header ends on a byte boundary
  // symbol spread and encoding table (FSE_buildCTable)
  uint8_t* tsym = h.fse_sym;
  uint16_t* st = h.fse_state;
  {
    const int step = (T >> 1) + (T >> 3) + 3;
    int pos = 0;
    for (int v = 0; v <= maxv; ++v)
      for (int i = 0; i < norm[v]; ++i) { tsym[pos] = (uint8_t)v; pos = (pos + step) & (T - 1); }
    int32_t* cumul = h.cumul;
    cumul[0] = 0;
    for (int v = 0; v < 16; ++v) cumul[v + 1] = cumul[v] + norm[v];
    for (int u = 0; u < T; ++u) st[cumul[tsym[u]]++] = (uint16_t)(T + u);
  }
  int32_t* dnb = h.dnb;
  int32_t* dfs = h.dfs;
  // (the first state of symbol v is cumul[v] - norm[v]: the table build above advanced cumul past v's states.  A
  //  running sum here instead was miscompiled for gfx950 -- dfs of the second symbol came out wrong.)
  for (int v = 0; v < 16; ++v) {
    if (!norm[v]) { dnb[v] = 0; dfs[v] = 0; continue; }
    if (norm[v] == 1) {
      dnb[v] = (L << 16) - T;
    } else {
      const int maxBitsOut = L - highbit((uint32_t)(norm[v] - 1));
      const int minStatePlus = norm[v] << maxBitsOut;
      dnb[v] = (maxBitsOut << 16) - minStatePlus;
    }
    dfs[v] = (h.cumul[v] - norm[v]) - norm[v];
  }
  auto init_state = [&](int v) -> uint32_t {
    const uint32_t nbo = (uint32_t)((dnb[v] + (1 << 15)) >> 16);
    const uint32_t val = (nbo << 16) - (uint32_t)dnb[v];
    return st[(val >> nbo) + dfs[v]];
  };
  auto encode = [&](uint32_t& state, int v) {
    const uint32_t nbo = (uint32_t)((int32_t)state + dnb[v]) >> 16;
    bw.add(state, (int)nbo);
    state = st[(state >> nbo) + dfs[v]];
  };
  // symbol i goes through state 1 when i is even, state 2 when odd; encoded last to first
  uint32_t s1, s2;
  int i = nw;
  if (nw & 1) {
    s1 = init_state(w[--i]);
    s2 = init_state(w[--i]);
    encode(s1, w[--i]);
  } else {
    s2 = init_state(w[--i]);
    s1 = init_state(w[--i]);
  }
  while (i > 0) {
    encode(s2, w[--i]);
    encode(s1, w[--i]);
  }
  bw.add(s2, L);
  bw.add(s1, L);
  const int n = bw.close();
  return n > 0 ? n : 0;
}

// The Huffman code of the literals counted in h (count, scount, sorted, nsym >= 2 filled): lengths, canonical codes,
// tree description, stream sizes.  Returns the bytes of tree description + jump table + four streams, 0 when the
// code cannot be written (a stream over 64 KiB, no tree description).  Single-threaded.
DSX_ZPLAN uint32_t plan_huffman(HufWork& h) {
  const int ns = h.nsym;
  for (int i = 0; i < ns; ++i) h.a[i] = h.sorted[i] >> 8;
  mk_lengths(h.a, ns);
  int* bl = h.bl;
  for (int l = 0; l <= kMaxBits; ++l) bl[l] = 0;
  for (int i = 0; i < ns; ++i) bl[h.a[i] > (uint32_t)kMaxBits ? kMaxBits : h.a[i]]++;
  int kraft = 0;
  for (int l = 1; l <= kMaxBits; ++l) kraft += bl[l] << (kMaxBits - l);
  while (kraft != (1 << kMaxBits)) {  // over-subscribed after the clamp: lengthen codes one unit at a time
    bl[kMaxBits]--;
    for (int l = kMaxBits - 1; l > 0; --l)
      if (bl[l]) { bl[l]--; bl[l + 1] += 2; break; }
    --kraft;
  }
  for (int s = 0; s < 256; ++s) h.len[s] = 0;
  {
    int i = 0;
    for (int l = kMaxBits; l >= 1; --l)
      for (int k = 0; k < bl[l]; ++k) h.len[h.sorted[i++] & 255u] = (uint8_t)l;
  }
  int mb = kMaxBits;
  while (!bl[mb]) --mb;
  h.max_bits = mb;
  {
    uint32_t* start = h.start;
    start[mb] = 0;
    for (int l = mb - 1; l >= 1; --l) start[l] = (start[l + 1] + (uint32_t)bl[l + 1]) >> 1;
    for (int s = 0; s < 256; ++s) h.code[s] = h.len[s] ? (uint16_t)start[h.len[s]]++ : 0;
  }
  int max_sym = 255;
  while (!h.len[max_sym]) --max_sym;
  for (int s = 0; s < 256; ++s) h.wgt[s] = h.len[s] ? (uint8_t)(mb + 1 - h.len[s]) : 0;
  const int nw = max_sym;  // weights described; the last one is implied
  const int direct = nw <= 128 ? 1 + (nw + 1) / 2 : 0;
  const int fse = fse_weights(h, h.wgt, nw, h.tree + 1, 127);
  if (fse > 0 && (direct == 0 || 1 + fse < direct)) {
    h.tree[0] = (uint8_t)fse;
    h.tree_bytes = 1 + fse;
  } else if (direct) {
    h.tree[0] = (uint8_t)(127 + nw);
    for (int i = 0; i < nw; i += 2) h.tree[1 + i / 2] = (uint8_t)((h.wgt[i] << 4) | (i + 1 < nw ? h.wgt[i + 1] : 0));
    h.tree_bytes = direct;
  } else {
    return 0;
  }
  uint32_t lit_c = (uint32_t)h.tree_bytes + 6;
  for (int k = 0; k < 4; ++k) {
    uint64_t bits = 0;
    for (int s = 0; s < 256; ++s) bits += (uint64_t)h.scount[k][s] * h.len[s];
    h.stream_bytes[k] = (uint32_t)(bits / 8 + 1);  // + the end mark
    if (k < 3 && h.stream_bytes[k] > 65535u) return 0;
    lit_c += h.stream_bytes[k];
  }
  return lit_c;
}

// The code of one block from its histograms (count, scount, sorted, nsym filled): lengths, canonical codes, tree
// description, stream sizes, block type and size.  Single-threaded.
DSX_ZPLAN void plan_block(HufWork& h, int n) {
  h.block_bytes = 3 + n;
  h.type = kRaw;
  h.prefix_bytes = 3;
  if (h.nsym == 1) {
    h.type = kRle;
    h.rle_byte = (uint8_t)(h.sorted[0] & 255u);
    h.block_bytes = 4;
    return;
  }
  if (n < kMinHuf) return;
  const uint32_t lit_c = plan_huffman(h);
  if (!lit_c) return;
  const uint32_t content = 5 + lit_c + 1;  // literals header + literals + sequences section (0 sequences)
  if (content >= (uint32_t)n) return;
  h.type = kCompressed;
  h.block_bytes = 3 + (int)content;
  h.prefix_bytes = 3 + 5 + h.tree_bytes + 6;
}

// Block header, literals header, tree description and jump table of a compressed block (prefix_bytes), and the
// sequences byte at its end; the four streams go in between.  For RLE / raw blocks: the 3-byte header (+ the byte).
DSX_ZPLAN void write_block_frame(const HufWork& h, int n, bool last, uint8_t* out) {
  if (h.type == kRle) {
    put_le(out, (uint32_t)last | (1u << 1) | ((uint32_t)n << 3), 3);
    out[3] = h.rle_byte;
    return;
  }
  if (h.type == kRaw) {
    put_le(out, (uint32_t)last | ((uint32_t)n << 3), 3);
    return;
  }
  const uint32_t content = (uint32_t)h.block_bytes - 3;
  put_le(out, (uint32_t)last | (2u << 1) | (content << 3), 3);
  const uint64_t lit_c = content - 5 - 1;
  put_le(out + 3, 2u | (3u << 2) | ((uint64_t)n << 4) | (lit_c << 22), 5);
  for (int i = 0; i < h.tree_bytes; ++i) out[8 + i] = h.tree[i];
  uint8_t* jt = out + 8 + h.tree_bytes;
  for (int k = 0; k < 3; ++k) put_le(jt + 2 * k, h.stream_bytes[k], 2);
  out[h.block_bytes - 1] = 0;
}

// ---- runs mode: the sequences of one block and the literals they leave --------------------------------------------
// Working state of the sequences of one zstd block (LDS on the device, ~10 KB).
struct SeqWork {
  uint32_t pos[kSeqCap], len[kSeqCap];  // the kept runs, ascending: first byte and length
  uint16_t st[3][64];                   // FSE encoding tables of the predefined distributions: 0 LL, 1 OF, 2 ML
  int32_t dnb[3][53], dfs[3][53];
  int32_t cumul[54];
  uint8_t tsym[64];
  int nseq, seq_bytes;
};

DSX_ZHD inline int ll_code(uint32_t v) {
  return v < 16 ? (int)v : v < 24 ? 16 + (int)((v - 16) >> 1) : v < 32 ? 20 + (int)((v - 24) >> 2)
         : v < 48 ? 22 + (int)((v - 32) >> 3) : v < 64 ? 24 : highbit(v) + 19;
}
DSX_ZHD inline int ml_code(uint32_t ml) {  // ml >= 3
  const uint32_t v = ml - 3;
  return v < 32 ? (int)v : v < 40 ? 32 + (int)((v - 32) >> 1) : v < 48 ? 36 + (int)((v - 40) >> 2)
         : v < 64 ? 38 + (int)((v - 48) >> 3) : v < 96 ? 40 + (int)((v - 64) >> 4) : v < 128 ? 42 : highbit(v) + 36;
}

// FSE encoding table of predefined distribution `which` (zstd's FSE_buildCTable; "less than 1" symbols take the top
// cells in symbol order, as build_fse of the decoder places them)
DSX_ZPLAN void build_seq_table(SeqWork& w, int which) {
  const int L = zdec::predefined_log(which), T = 1 << L, ns = zdec::predefined_symbols(which);
  int high = T - 1;
  w.cumul[0] = 0;
  for (int s = 0; s < ns; ++s) {
    const int nm = zdec::predefined_norm(which, s);
    w.cumul[s + 1] = w.cumul[s] + (nm < 0 ? 1 : nm);
    if (nm < 0) w.tsym[high--] = (uint8_t)s;
  }
  const int step = (T >> 1) + (T >> 3) + 3;
  int at = 0;
  for (int s = 0; s < ns; ++s) {
    const int nm = zdec::predefined_norm(which, s);
    for (int i = 0; i < nm; ++i) {
      w.tsym[at] = (uint8_t)s;
      do at = (at + step) & (T - 1);
      while (at > high);
    }
  }
  for (int s = 0; s < ns; ++s) {
    const int nm = zdec::predefined_norm(which, s), c = nm < 0 ? 1 : nm;
    if (c == 1) {
      w.dnb[which][s] = (L << 16) - T;
    } else {
      const int maxBitsOut = L - highbit((uint32_t)(c - 1));
      w.dnb[which][s] = (maxBitsOut << 16) - (c << maxBitsOut);
    }
    w.dfs[which][s] = w.cumul[s] - c;
  }
  for (int u = 0; u < T; ++u) w.st[which][w.cumul[w.tsym[u]]++] = (uint16_t)(T + u);
}
DSX_ZHD inline uint32_t seq_state(const SeqWork& w, int which, int sym) {  // FSE_initCState2
  const int32_t d = w.dnb[which][sym];
  const uint32_t nbo = (uint32_t)((d + (1 << 15)) >> 16);
  const uint32_t val = (nbo << 16) - (uint32_t)d;
  return w.st[which][(int32_t)(val >> nbo) + w.dfs[which][sym]];
}
DSX_ZHD inline void seq_symbol(const SeqWork& w, int which, BitW& bw, uint32_t& state, int sym) {  // FSE_encodeSymbol
  const uint32_t nbo = (uint32_t)((int32_t)state + w.dnb[which][sym]) >> 16;
  bw.add(state, (int)nbo);
  state = w.st[which][(int32_t)(state >> nbo) + w.dfs[which][sym]];
}

// Sequences section of the runs w.pos / w.len [0 .. w.nseq), nseq >= 1 -> out: Number_of_Sequences, the modes byte
// (all predefined), the bit stream.  Sequence k: literal length = bytes from the end of run k - 1 to the first byte of
// run k inclusive, match length = len - 1, offset code 0 (Offset_Value 1).  Returns the bytes, -1 when they exceed cap.
// Single-threaded.
DSX_ZPLAN int encode_sequences(SeqWork& w, uint8_t* out, int cap) {
  static_assert(kSeqCap < 0x7F00, "Number_of_Sequences is written in one or two bytes");
  static_assert(kMinRun >= 4, "a match is at least 3 bytes");
  const int nseq = w.nseq;
  if (cap < 4) return -1;
  for (int t = 0; t < 3; ++t) build_seq_table(w, t);
  int p = 0;
  if (nseq < 128) {
    out[p++] = (uint8_t)nseq;
  } else {
    out[p++] = (uint8_t)((nseq >> 8) + 128);
    out[p++] = (uint8_t)nseq;
  }
  out[p++] = 0;  // Predefined_Mode x 3
  BitW bw(out + p, cap - p);
  int k = nseq - 1;
  uint32_t ll = w.pos[k] + 1 - (k ? w.pos[k - 1] + w.len[k - 1] : 0u), ml = w.len[k] - 1;
  int lc = ll_code(ll), mc = ml_code(ml);
  uint32_t sml = seq_state(w, 2, mc), sof = seq_state(w, 1, 0), sll = seq_state(w, 0, lc);
  bw.add(ll - zdec::ll_base(lc), zdec::ll_bits(lc));
  bw.add(ml - zdec::ml_base(mc), zdec::ml_bits(mc));
  for (--k; k >= 0; --k) {
    ll = w.pos[k] + 1 - (k ? w.pos[k - 1] + w.len[k - 1] : 0u);
    ml = w.len[k] - 1;
    lc = ll_code(ll);
    mc = ml_code(ml);
    seq_symbol(w, 1, bw, sof, 0);
    seq_symbol(w, 2, bw, sml, mc);
    seq_symbol(w, 0, bw, sll, lc);
    bw.add(ll - zdec::ll_base(lc), zdec::ll_bits(lc));
    bw.add(ml - zdec::ml_base(mc), zdec::ml_bits(mc));
  }
  bw.add(sml, zdec::predefined_log(2));
  bw.add(sof, zdec::predefined_log(1));
  bw.add(sll, zdec::predefined_log(0));
  const int n = bw.close();
  return n < 0 ? -1 : p + n;
}

// Literals section of nl >= 1 literals counted in h (as for plan_block): h.type = its form (kRle, kRaw, or kCompressed
// = Huffman), h.block_bytes = its bytes with the header, h.prefix_bytes = the bytes in front of the literal bytes /
// the four streams.  The smallest form; ties: RLE, raw, Huffman.  Single-threaded.  (With maximal runs two neighbouring
// stretches differ, so literals of one value mean one literal: the RLE form is here for completeness of the plan.)
DSX_ZHD inline int lit_header_bytes(int nl) { return nl < 32 ? 1 : (nl < 4096 ? 2 : 3); }
DSX_ZPLAN void plan_literals(HufWork& h, int nl) {
  const int hb = lit_header_bytes(nl);
  h.prefix_bytes = hb;
  if (h.nsym == 1) {
    h.type = kRle;
    h.rle_byte = (uint8_t)(h.sorted[0] & 255u);
    h.block_bytes = hb + 1;
    return;
  }
  h.type = kRaw;
  h.block_bytes = hb + nl;
  if (nl < kMinHuf) return;
  const uint32_t lit_c = plan_huffman(h);
  if (!lit_c || 5 + lit_c >= (uint32_t)h.block_bytes) return;
  h.type = kCompressed;
  h.block_bytes = 5 + (int)lit_c;
  h.prefix_bytes = 5 + h.tree_bytes + 6;
}
// h.prefix_bytes at out (+ the byte of an RLE section)
DSX_ZPLAN void write_literals_head(const HufWork& h, int nl, uint8_t* out) {
  if (h.type == kCompressed) {
    const uint64_t lit_c = (uint64_t)h.block_bytes - 5;
    put_le(out, 2u | (3u << 2) | ((uint64_t)nl << 4) | (lit_c << 22), 5);
    for (int i = 0; i < h.tree_bytes; ++i) out[5 + i] = h.tree[i];
    for (int k = 0; k < 3; ++k) put_le(out + 5 + h.tree_bytes + 2 * k, h.stream_bytes[k], 2);
    return;
  }
  const uint32_t t = h.type == kRle ? 1u : 0u, hb = (uint32_t)h.prefix_bytes;
  if (hb == 1) out[0] = (uint8_t)(t | ((uint32_t)nl << 3));
  else put_le(out, t | ((hb == 2 ? 1u : 3u) << 2) | ((uint32_t)nl << 4), (int)hb);
  if (h.type == kRle) out[hb] = h.rle_byte;
}
// Bytes of the block in runs mode from the two planned sections (seq_bytes < 0: the sequences did not fit)
DSX_ZHD inline int runs_block_bytes(const HufWork& h2, int seq_bytes) { return 3 + h2.block_bytes + seq_bytes; }
DSX_ZHD inline void write_runs_block_header(int block_bytes, bool last, uint8_t* out) {
  put_le(out, (uint32_t)last | (2u << 1) | ((uint32_t)(block_bytes - 3) << 3), 3);
}

// zstd frame header of a frame with `size` bytes of content (single segment, no checksum, no dictionary)
DSX_ZHD inline int frame_header(uint32_t size, uint8_t* out) {
  put_le(out, 0xFD2FB528u, 4);
  if (size < 256) { out[4] = 0x20; out[5] = (uint8_t)size; return 6; }
  if (size < 65536 + 256) { out[4] = 0x60; put_le(out + 5, size - 256, 2); return 7; }
  out[4] = 0xA0;
  put_le(out + 5, size, 4);
  return 9;
}
DSX_ZHD inline int frame_header_bytes(uint32_t size) { return size < 256 ? 6 : (size < 65536 + 256 ? 7 : 9); }

constexpr int kZPerBlosc = kSlotsPerBlock;  // zstd blocks per Blosc block (at most): one slot each
static_assert(kZPerBlosc * kZBlock == kBloscBlock && kSlotStride >= 3 + kZBlock, "a zstd block fits its slot");

// The container of the zstd modes (dsx_blosc_frame.h): "don't split", so a Blosc block is one stream -- a zstd frame
// header and the zstd blocks of its slots, stored when that is not below the block.
struct ZstdFrames {
  static constexpr unsigned kFlags = kBloscShuffle | kBloscDontSplit | (kInnerZstd << 5);
  static constexpr int kParts = kZPerBlosc;
  DSX_ZHD static int streams(const Geometry&, uint64_t, int) { return 1; }
  DSX_ZHD static uint32_t stream_bytes(const uint32_t* zs, uint32_t bsize, int) {
    uint32_t f = (uint32_t)frame_header_bytes(bsize);
    for (int j = 0; j < kZPerBlosc; ++j) f += zs[j];
    return f < bsize ? f : bsize;
  }
  DSX_ZHD static int prefix(uint32_t bsize, uint8_t* out) { return frame_header(bsize, out); }
  DSX_ZHD static int prefix_bytes(uint32_t bsize) { return frame_header_bytes(bsize); }
};

// ---- host build: one zstd block, and whole chunks ------------------------------------------------------------
// histograms, symbol count and sort of lit[0 .. n) -> h
inline void count_host(HufWork& h, const uint8_t* lit, int n) {
  for (int k = 0; k < 4; ++k) {
    for (int s = 0; s < 256; ++s) h.scount[k][s] = 0;
    for (int i = stream_begin(n, k); i < stream_begin(n, k + 1); ++i) h.scount[k][lit[i]]++;
  }
  h.nsym = 0;
  for (int s = 0; s < 256; ++s) {
    h.count[s] = h.scount[0][s] + h.scount[1][s] + h.scount[2][s] + h.scount[3][s];
    h.nsym += h.count[s] != 0;
  }
  for (int s = 0; s < 256; ++s) if (h.count[s]) h.sorted[sort_rank(h, s)] = sort_key(h, s);
}
// the four Huffman streams of lit[0 .. n) -> dst
inline void pack_streams_host(const HufWork& h, const uint8_t* lit, int n, uint8_t* dst) {
  for (int k = 0; k < 4; ++k) {
    BitW bw(dst, (int)h.stream_bytes[k]);
    for (int i = stream_begin(n, k + 1) - 1; i >= stream_begin(n, k); --i) bw.add(h.code[lit[i]], h.len[lit[i]]);
    bw.close();
    dst += h.stream_bytes[k];
  }
}
// literals lit[0 .. n) -> slot (block header included); returns the block's bytes.  h: caller's work space.
inline int encode_block_host(HufWork& h, const uint8_t* lit, int n, bool last, uint8_t* slot) {
  count_host(h, lit, n);
  plan_block(h, n);
  write_block_frame(h, n, last, slot);
  if (h.type == kRaw) {
    for (int i = 0; i < n; ++i) slot[3 + i] = lit[i];
  } else if (h.type == kCompressed) {
    pack_streams_host(h, lit, n, slot + h.prefix_bytes);
  }
  return h.block_bytes;
}

// Work space of the host build in runs mode
struct RunsHost {
  HufWork h2;
  SeqWork w;
  uint8_t work[kSlotStride];  // the literals the runs leave, the sequences section behind them
};
// The same in runs mode: the entropy-only block first, then the block with sequences where that one is smaller.
inline int encode_block_runs_host(HufWork& h, RunsHost& r, const uint8_t* lit, int n, bool last, uint8_t* slot) {
  const int bytes0 = encode_block_host(h, lit, n, last, slot);
  if (h.type == kRle) return bytes0;
  SeqWork& w = r.w;
  w.nseq = 0;
  for (int i = 0; i < n;) {
    int e = i + 1;
    while (e < n && lit[e] == lit[i]) ++e;
    if (e - i >= kMinRun && w.nseq < kSeqCap) {
      w.pos[w.nseq] = (uint32_t)i;
      w.len[w.nseq++] = (uint32_t)(e - i);
    }
    i = e;
  }
  if (!w.nseq) return bytes0;
  int nl = 0, at = 0;
  for (int k = 0; k < w.nseq; ++k) {
    for (int i = at; i <= (int)w.pos[k]; ++i) r.work[nl++] = lit[i];
    at = (int)(w.pos[k] + w.len[k]);
  }
  for (int i = at; i < n; ++i) r.work[nl++] = lit[i];
  count_host(r.h2, r.work, nl);
  plan_literals(r.h2, nl);
  w.seq_bytes = encode_sequences(w, r.work + nl, kSlotStride - nl);
  const int bytes1 = runs_block_bytes(r.h2, w.seq_bytes);
  if (w.seq_bytes < 0 || bytes1 >= bytes0) return bytes0;
  write_runs_block_header(bytes1, last, slot);
  write_literals_head(r.h2, nl, slot + 3);
  uint8_t* d = slot + 3 + r.h2.prefix_bytes;
  if (r.h2.type == kRaw) {
    for (int i = 0; i < nl; ++i) d[i] = r.work[i];
  } else if (r.h2.type == kCompressed) {
    pack_streams_host(r.h2, r.work, nl, d);
  }
  for (int i = 0; i < w.seq_bytes; ++i) slot[3 + r.h2.block_bytes + i] = r.work[nl + i];
  return bytes1;
}

// n_chunks chunks of chunk_bytes (uint16) -> packed frames + offsets[n_chunks + 1] (the device encoder's output).
// frames: n_chunks * (chunk_bytes + 16) bytes at most.
inline void blosc_encode_host(const uint16_t* src, uint64_t n_chunks, uint64_t chunk_bytes, int clevel,
                              uint8_t* frames, int64_t* offsets, int mode = kModeLiterals) {
  HufWork* h = new HufWork;
  RunsHost* runs = mode == kModeRuns ? new RunsHost : nullptr;
  assemble_chunks_host<ZstdFrames>(src, n_chunks, chunk_bytes, clevel, frames, offsets,
                                   [&](const uint8_t* lit, uint32_t bsize, int, uint8_t* slots, uint32_t* zs) {
    for (int j = 0; j < kZPerBlosc && (uint32_t)j * kZBlock < bsize; ++j) {
      const uint32_t z0 = (uint32_t)j * kZBlock, z1 = bsize - z0 < (uint32_t)kZBlock ? bsize : z0 + kZBlock;
      uint8_t* sl = slots + (size_t)j * kSlotStride;
      zs[j] = (uint32_t)(runs ? encode_block_runs_host(*h, *runs, lit + z0, (int)(z1 - z0), z1 == bsize, sl)
                              : encode_block_host(*h, lit + z0, (int)(z1 - z0), z1 == bsize, sl));
    }
  });
  delete runs;
  delete h;
}

}  // namespace zenc
}  // namespace dsx

#endif  // DSX_ZSTD_ENC_H
