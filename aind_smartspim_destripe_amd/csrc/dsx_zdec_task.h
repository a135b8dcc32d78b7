// dsx_zdec_task.h -- the task model of the Blosc block decoder: what dsx_io_read_frames writes, what the host
// reference (dsx_blosc_decode_ref -> run_task_host) and the device kernels (dsx_zdec_kernels.h zdec_task) run.  The
// codecs themselves are one header each (dsx_zstd_dec.h, dsx_lz4_dec.h, dsx_inflate.h: format primitives shared by
// both builds, and a host decoder of one stream); here is everything around a stream.  Plain C++ with no STL, no
// allocation and no library call; g++ builds it for the CPU tests (tests/host/zdec_task_check.cpp, also under ASan /
// UBSan).
//
// A task makes dst_len bytes of output from src_len packed bytes:
//   kind & 0xFF  kTaskFill: the 16-bit value in `src` repeated.  kTaskCopy / kTaskStored: the bytes themselves.
//                kTaskZstd / kTaskLz4 / kTaskZlib / kTaskBlosclz: one stream of that codec.  Anything else is refused.
//   kTaskSplit   the bytes are two streams behind an int32 length each, for the low-byte and the high-byte half of the
//                output; a stream as long as its half is stored.  Only with a codec kind.
//   kTaskShuffle / kTaskBitshuffle   the byte / bit un-shuffle of 2-byte elements follows (bit wins over byte).
// Other bits of `kind` mean nothing.  engine.py and the golden tables of the tests hold these numbers.
#ifndef DSX_ZDEC_TASK_H
#define DSX_ZDEC_TASK_H

#include "dsx_inflate.h"
#include "dsx_lz4_dec.h"
#include "dsx_zstd_dec.h"

namespace dsx {
namespace zdec {

enum TaskKind { kTaskFill = 0, kTaskCopy = 1, kTaskStored = 2, kTaskZstd = 3 };
constexpr uint32_t kTaskLz4 = 4;      // one bare LZ4 block
constexpr uint32_t kTaskZlib = 5;     // one zlib stream (RFC 1950)
constexpr uint32_t kTaskBlosclz = 6;  // one blosclz stream
constexpr uint32_t kTaskKindMask = 0xFF;
constexpr uint32_t kTaskShuffle = 0x100;     // byte un-shuffle of 2-byte elements after the copy / decode
constexpr uint32_t kTaskSplit = 0x200;       // src is the int32 length word of the first of 2 streams of the kind
constexpr uint32_t kTaskBitshuffle = 0x400;  // bit un-shuffle of 2-byte elements after the decode
constexpr uint32_t kSplitStreams = 2;        // typesize 2: one stream of low bytes, one of high bytes

struct DecTask {
  uint64_t src;      // offset of the bytes in the packed buffer (kTaskFill: the 16-bit fill value)
  uint64_t dst;      // offset in the output
  uint32_t src_len;  // bytes in the packed buffer
  uint32_t dst_len;  // bytes of output
  uint32_t kind;     // kind | flags
  uint32_t chunk;    // index of the chunk file (error messages)
};

// the tables of one task: a zstd frame or a zlib stream (LDS on the device)
union DecWork {
  Tables t;
  InfTables inf;
};
static_assert(sizeof(InfTables) <= sizeof(Tables), "the inflate tables live in the space of the zstd tables");

// The watermark rule of the device drivers.  Output below `fenced` was made visible to the wave by its last barrier.
// A match whose source starts at src, `off` bytes behind its destination, loads the bytes [src, src + min(ml, off))
// (the rest of a longer match repeats them): when they reach above the watermark, a barrier comes first.
DSX_ZHD inline bool match_needs_fence(uint32_t src, uint32_t ml, uint32_t off, uint32_t fenced) {
  return src + (ml < off ? ml : off) > fenced;
}

// ---- split streams --------------------------------------------------------------------------------------------------
// The next stream of a split block at s + *pos (n bytes in all): its int32 length, then its bytes.  Returns a status;
// on kOk *at / *len are the stream's bytes and *pos is past them.
DSX_ZHD inline int split_stream(const uint8_t* s, uint32_t n, uint32_t* pos, uint32_t* at, uint32_t* len) {
  if (*pos > n || n - *pos < 4) return kErrTruncated;
  const uint32_t cs = le(s + *pos, 4);
  if (cs > n - *pos - 4) return kErrTruncated;
  *at = *pos + 4;
  *len = cs;
  *pos += 4 + cs;
  return kOk;
}

// ---- byte un-shuffle ------------------------------------------------------------------------------------------------
// byte p of the un-shuffled output from the shuffled block s of n bytes (2-byte elements, the odd tail as is)
DSX_ZHD inline uint8_t unshuffled_byte(const uint8_t* s, uint32_t n, uint32_t p) {
  const uint32_t ne = n / 2;
  return p < 2 * ne ? s[(p & 1) * ne + (p >> 1)] : s[p];
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

// ---- one task on the host ---------------------------------------------------------------------------------------------
// The flow of zdec_task (dsx_zdec_kernels.h), statement for statement; the caller has checked that the task's bytes
// and its output lie in their buffers.  tmp: dst_len bytes of scratch.  Returns a status.
inline int run_task_host(DecWork& wk, const DecTask& k, const uint8_t* packed, uint8_t* out, uint8_t* tmp) {
  const uint32_t kind = k.kind & kTaskKindMask;
  const bool split = (k.kind & kTaskSplit) != 0, bits = (k.kind & kTaskBitshuffle) != 0;
  const bool shuf = !bits && (k.kind & kTaskShuffle) != 0;
  const uint32_t out_n = k.dst_len, n = k.src_len;
  uint8_t* d = out + k.dst;
  if (kind == kTaskFill) {
    for (uint32_t i = 0; i < out_n; ++i) d[i] = (uint8_t)(k.src >> (8 * (i & 1)));
    return kOk;
  }
  const uint8_t* s = packed + k.src;
  const bool plain = !split && (kind == kTaskCopy || kind == kTaskStored);  // the bytes are there: un-shuffle or copy
  if (!plain && (kind < kTaskZstd || kind > kTaskBlosclz)) return kErrReserved;
  uint8_t* o = (shuf || bits) ? tmp : d;
  // the streams of the block one after the other, each into its share of the block: a split block holds a low-byte
  // and a high-byte stream behind an int32 length each (a length of the whole share: stored), any other block is
  // its one stream
  const uint32_t nstreams = split ? kSplitStreams : 1u;
  const uint32_t ne = out_n / nstreams;
  if (out_n % nstreams) return kErrOutput;
  if (plain && n != out_n) return kErrOutput;
  uint32_t pos = 0;
  for (uint32_t j = 0; j < nstreams && !plain; ++j) {
    uint32_t at = 0, len = n;
    int st = split ? split_stream(s, n, &pos, &at, &len) : kOk;
    if (st) return st;
    if (split && len == ne) copy_bytes(o + j * ne, s + at, ne);  // stored
    else if (kind == kTaskZstd) st = decode_frame(wk.t, s + at, len, o + j * ne, ne);
    else if (kind == kTaskLz4) st = lz4_decode(s + at, len, o + j * ne, ne);
    else if (kind == kTaskZlib) st = inflate_decode(wk.inf, s + at, len, o + j * ne, ne);
    else st = blosclz_decode(s + at, len, o + j * ne, ne);
    if (st) return st;
  }
  if (split && pos != n) return kErrTruncated;
  const uint8_t* from = plain ? s : o;
  if (bits) unbitshuffle_host(d, from, out_n);
  else if (shuf)
    for (uint32_t i = 0; i < out_n; ++i) d[i] = unshuffled_byte(from, out_n, i);
  else if (plain) copy_bytes(d, s, n);
  return kOk;
}

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_ZDEC_TASK_H
