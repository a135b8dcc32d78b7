// dsx_lz4_dec.h -- what the device decoder needs beyond unsplit zstd frames (DSX_ZDEC_ANY): bare LZ4 blocks, the
// split streams of a c-blosc block and the bit un-shuffle of 2-byte elements.  Shared by the host reference
// (dsx_blosc_decode_ref) and the device kernel (dsx_zdec_kernels.h), like dsx_zstd_dec.h: plain C++ with no STL, no
// allocation and no library call; g++ builds it for the CPU tests (tests/host/lz4_dec_check.cpp, also under ASan /
// UBSan).
//
// LZ4 block format (lz4_Block_format.md): a block is a series of sequences.  A sequence is a token (high nibble:
// literal length, low nibble: match length - 4; a nibble of 15 is followed by extension bytes that add up until one
// is not 255), the literals, a 2-byte little-endian match offset and the match-length extension bytes.  The last
// sequence ends after its literals.  A match may overlap its own output (offset < length): it then repeats the last
// `offset` bytes.  c-blosc stores such blocks bare, the output size comes from the Blosc header.
//
// Safety: lz4_next validates a whole sequence against the input and the output before a byte of it is copied; a
// malformed stream ends in a status of dsx_zstd_dec.h, never in an access outside either buffer.
#ifndef DSX_LZ4_DEC_H
#define DSX_LZ4_DEC_H

#include "dsx_zstd_dec.h"

namespace dsx {
namespace zdec {

// task kinds and flags next to those of dsx_zstd_dec.h (TaskKind 0 .. 3, kTaskShuffle = 0x100)
constexpr uint32_t kTaskLz4 = 4;             // one bare LZ4 block
constexpr uint32_t kTaskSplit = 0x200;       // src is the int32 length word of the first of 2 streams of the kind
constexpr uint32_t kTaskBitshuffle = 0x400;  // bit un-shuffle of 2-byte elements after the decode
constexpr uint32_t kSplitStreams = 2;        // typesize 2: one stream of low bytes, one of high bytes

struct Lz4Seq {
  uint32_t lit;  // where the literals start in the stream
  uint32_t ll, ml, off;  // ml == 0: the last sequence (literals only)
};

// reads the stream bytes for lz4_next: the host reads them in place, the device through a window in LDS
struct Lz4Direct {
  const uint8_t* s;
  DSX_ZHD uint8_t at(uint32_t p) { return s[p]; }
};

// The sequence at ip of a stream of n bytes whose output so far is op of out_n bytes: validated, then ip and op are
// moved past it as if it had been executed.  Returns a status.
template <typename R>
DSX_ZHD inline int lz4_next(R& r, uint32_t n, uint32_t out_n, uint32_t& ip, uint32_t& op, Lz4Seq& q) {
  if (ip >= n) return kErrTruncated;  // (a stream never ends on a match)
  const uint32_t token = r.at(ip++);
  uint32_t ll = token >> 4;
  if (ll == 15) {
    uint32_t b;
    do {
      if (ip >= n) return kErrTruncated;
      b = r.at(ip++);
      ll += b;
      if (ll > out_n) return kErrOutput;
    } while (b == 255);
  }
  if (ll > n - ip) return kErrTruncated;
  if (ll > out_n - op) return kErrOutput;
  q.lit = ip;
  q.ll = ll;
  ip += ll;
  op += ll;
  if (ip == n) {
    q.ml = 0;
    q.off = 0;
    return kOk;
  }
  if (n - ip < 2) return kErrTruncated;
  const uint32_t off = (uint32_t)r.at(ip) | ((uint32_t)r.at(ip + 1) << 8);
  ip += 2;
  uint32_t ml = token & 15;
  if (ml == 15) {
    uint32_t b;
    do {
      if (ip >= n) return kErrTruncated;
      b = r.at(ip++);
      ml += b;
      if (ml > out_n) return kErrOutput;
    } while (b == 255);
  }
  ml += 4;
  if (off == 0 || off > op) return kErrOffset;
  if (ml > out_n - op) return kErrOutput;
  q.ml = ml;
  q.off = off;
  op += ml;
  return kOk;
}

// ---- host build: one whole block -----------------------------------------------------------------------------------
// Stream s[0 .. n) -> out[0 .. out_n), exactly.
inline int lz4_decode(const uint8_t* s, uint32_t n, uint8_t* out, uint32_t out_n) {
  Lz4Direct r{s};
  uint32_t ip = 0, op = 0;
  for (;;) {
    Lz4Seq q;
    uint32_t at = op;
    const int st = lz4_next(r, n, out_n, ip, op, q);
    if (st) return st;
    for (uint32_t i = 0; i < q.ll; ++i) out[at + i] = s[q.lit + i];
    if (q.ml == 0) break;
    uint8_t* d = out + at + q.ll;
    for (uint32_t i = 0; i < q.ml; ++i) d[i] = d[(int64_t)i - (int64_t)q.off];
  }
  return op == out_n ? kOk : kErrOutput;
}

// ---- bit un-shuffle of 2-byte elements -----------------------------------------------------------------------------
// c-blosc's bit shuffle of a block of ne = n / 2 elements, ne a multiple of 8: 16 rows of ne / 8 bytes, row 8 s + b =
// bit b of byte s of every element, element 8 j + k in bit k of byte j.  Any other block is left as it is (c-blosc
// 1.21 shuffle.c, blosc_unbitshuffle of dsx_io.h).
DSX_ZHD inline bool bitshuffled(uint32_t n) { return n / 2 != 0 && ((n / 2) & 7u) == 0; }

// 8 x 8 bit matrix, byte i bit j <-> byte j bit i (bit 0 = least significant)
DSX_ZHD inline uint64_t transpose8(uint64_t x) {
  uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
  x ^= t ^ (t << 7);
  t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
  x ^= t ^ (t << 14);
  t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
  x ^= t ^ (t << 28);
  return x;
}

// elements 8 j .. 8 j + 7 (16 bytes at d + 16 j) of the shuffled block s whose rows are `row` bytes
DSX_ZHD inline void unbitshuffle8(const uint8_t* s, uint32_t row, uint32_t j, uint64_t* lo, uint64_t* hi) {
  uint64_t a = 0, b = 0;
  for (int r = 0; r < 8; ++r) {
    a |= (uint64_t)s[(uint32_t)r * row + j] << (8 * r);
    b |= (uint64_t)s[(uint32_t)(8 + r) * row + j] << (8 * r);
  }
  a = transpose8(a);  // byte k = low byte of element 8 j + k
  b = transpose8(b);  // byte k = its high byte
  uint64_t w0 = 0, w1 = 0;
  for (int k = 0; k < 4; ++k) {
    w0 |= (((a >> (8 * k)) & 0xFFull) | (((b >> (8 * k)) & 0xFFull) << 8)) << (16 * k);
    w1 |= (((a >> (8 * (k + 4))) & 0xFFull) | (((b >> (8 * (k + 4))) & 0xFFull) << 8)) << (16 * k);
  }
  *lo = w0;
  *hi = w1;
}

inline void unbitshuffle_host(uint8_t* d, const uint8_t* s, uint32_t n) {
  if (!bitshuffled(n)) {
    for (uint32_t i = 0; i < n; ++i) d[i] = s[i];
    return;
  }
  const uint32_t row = n / 16;
  for (uint32_t j = 0; j < row; ++j) {
    uint64_t w[2];
    unbitshuffle8(s, row, j, &w[0], &w[1]);
    for (int i = 0; i < 16; ++i) d[16 * j + (uint32_t)i] = (uint8_t)(w[i >> 3] >> (8 * (i & 7)));
  }
  if (n & 1u) d[n - 1] = s[n - 1];
}

// ---- split streams --------------------------------------------------------------------------------------------------
// Stream j of a split block at s + *pos (n bytes in all): its int32 length, then its bytes.  Returns a status; on
// kOk *at / *len are the stream's bytes and *pos is past them.
DSX_ZHD inline int split_stream(const uint8_t* s, uint32_t n, uint32_t* pos, uint32_t* at, uint32_t* len) {
  if (*pos > n || n - *pos < 4) return kErrTruncated;
  const uint32_t cs = le(s + *pos, 4);
  if (cs > n - *pos - 4) return kErrTruncated;
  *at = *pos + 4;
  *len = cs;
  *pos += 4 + cs;
  return kOk;
}

// One stream of `kind` on the host: len bytes at s -> out_n bytes at o (len == out_n in a split block: stored)
inline int run_stream_host(Tables& t, uint32_t kind, bool split, const uint8_t* s, uint32_t len, uint8_t* o,
                           uint32_t out_n) {
  if ((split && len == out_n) || kind == kTaskCopy || kind == kTaskStored) {
    if (len != out_n) return kErrOutput;
    for (uint32_t i = 0; i < out_n; ++i) o[i] = s[i];
    return kOk;
  }
  if (kind == kTaskZstd) return decode_frame(t, s, len, o, out_n);
  if (kind == kTaskLz4) return lz4_decode(s, len, o, out_n);
  return kErrReserved;
}

// One task of any kind on the host; tmp: dst_len bytes of scratch.  Tasks of dsx_zstd_dec.h's kinds and flags run
// through run_task_host as before.  Returns a status.
inline int run_task_host_any(Tables& t, const DecTask& k, const uint8_t* packed, uint8_t* out, uint8_t* tmp) {
  const uint32_t kind = k.kind & kTaskKindMask;
  if (kind <= kTaskZstd && !(k.kind & ~(kTaskKindMask | kTaskShuffle))) return run_task_host(t, k, packed, out, tmp);
  if (kind == kTaskFill) return run_task_host(t, k, packed, out, tmp);
  const bool split = (k.kind & kTaskSplit) != 0, bits = (k.kind & kTaskBitshuffle) != 0;
  if (kind > kTaskLz4 || (split && kind != kTaskZstd && kind != kTaskLz4)) return kErrReserved;
  const bool shuf = !bits && (k.kind & kTaskShuffle) != 0;
  const uint8_t* s = packed + k.src;
  uint8_t* d = out + k.dst;
  uint8_t* o = (shuf || bits) ? tmp : d;
  if (split) {
    if (k.dst_len % kSplitStreams) return kErrOutput;
    const uint32_t ne = k.dst_len / kSplitStreams;
    uint32_t pos = 0;
    for (uint32_t j = 0; j < kSplitStreams; ++j) {
      uint32_t at = 0, len = 0;
      int st = split_stream(s, k.src_len, &pos, &at, &len);
      if (!st) st = run_stream_host(t, kind, true, s + at, len, o + j * ne, ne);
      if (st) return st;
    }
    if (pos != k.src_len) return kErrTruncated;
  } else {
    const int st = run_stream_host(t, kind, false, s, k.src_len, o, k.dst_len);
    if (st) return st;
  }
  if (bits) unbitshuffle_host(d, o, k.dst_len);
  else if (shuf)
    for (uint32_t i = 0; i < k.dst_len; ++i) d[i] = unshuffled_byte(o, k.dst_len, i);
  return kOk;
}

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_LZ4_DEC_H
