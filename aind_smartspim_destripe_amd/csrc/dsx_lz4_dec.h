// dsx_lz4_dec.h -- bare LZ4 blocks for the Blosc block decoder (task kind kTaskLz4 of dsx_zdec_task.h): lz4_next, the
// sequence parser shared by the host reference (dsx_blosc_decode_ref) and the device kernel (dsx_zdec_kernels.h), and
// lz4_decode, the host decoder of one block.  Like dsx_zstd_dec.h: plain C++ with no STL, no allocation and no library
// call; g++ builds it for the CPU tests (tests/host/zdec_task_check.cpp, also under ASan / UBSan).
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
    const uint32_t at = op;
    const int st = lz4_next(r, n, out_n, ip, op, q);
    if (st) return st;
    run_seq_host(out + at, s + q.lit, q.ll, q.ml, q.off);
    if (q.ml == 0) break;
  }
  return op == out_n ? kOk : kErrOutput;
}

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_LZ4_DEC_H
