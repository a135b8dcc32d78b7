// dsx_lz4_enc.h -- LZ4 blocks inside Blosc frames: the encoder core shared by the host build (the I/O threads'
// Blosc-LZ4 writer, dsx_blosc_encode_ref_ex) and the device kernels (dsx_lz4enc_kernels.h).  Plain C++; g++ builds it
// for the CPU tests (tests/host/lz4_enc_check.cpp).
//
// Stream format (LZ4 block format, not the frame format): sequences of token (literal length << 4 | match length - 4),
// literal length bytes (255-chained from 15 on), literals, 2-byte offset, match length bytes (the same chaining).  The
// last sequence is literals only.  Held rules: a stream under 13 bytes is literals only, the last 5 bytes are literals,
// no match starts within the last 12 bytes, offsets 1 ... 65 535, matches >= 4 bytes.
//
// The finder is a function of the stream's bytes alone, so the kernel writes the bytes of the host build: a table of
// kTable positions keyed by a multiplicative hash of the 4 bytes at a position, walked in groups of kGroup consecutive
// positions from a cursor.  Every position of the group looks its candidate up first, then all are entered (an entry
// keeps the highest position ever entered under its key: entries only grow, which a later group overwriting an earlier
// one would give as well, because the positions a group repeats carry the keys they had).  The first position of the
// group whose candidate verifies (strictly below the position -- after a match the table already holds positions at
// and behind the new cursor --, distance <= 65 535, 4 equal bytes) opens a match; it is extended to the first mismatch
// or to 5 bytes before the end; the cursor goes to its end.  Without a match the cursor advances by kGroup.  No
// backward extension, no entries inside matches.
//
// A stream that does not shrink is "stored": the encoder gives up as soon as the bytes written plus the literals owed
// (anchor ... cursor) reach the stream's length, and a sequence is only written while the output stays below it, so a
// slot of the stream's own length always suffices and noise costs one scan.
//
// Blosc container: what c-blosc 1.21 writes for LZ4 with byte shuffle at typesize 2 -- version 2, versionlz 1, flags
// SHUFFLE | (1 << 5) ("don't split" clear), 256 KiB blocks.  A full block is two streams, the low-byte plane and the
// high-byte plane, each with its int32 length and each coded or stored (length == plane length) on its own; a short
// last block (leftover) is one stream.  A chunk under 128 bytes, clevel 0, or a frame not smaller than its data is a
// memcpyed frame.
#ifndef DSX_LZ4_ENC_H
#define DSX_LZ4_ENC_H

#include <stddef.h>
#include <stdint.h>

#include "dsx_blosc_frame.h"  // the container: Geometry, shuffled_byte, put_le, the slots, assemble_chunk_host

namespace dsx {
namespace lz4enc {

using namespace blosc;

constexpr int kGroup = 64;                 // positions per step (one wave)
constexpr int kHashLog = 12;
constexpr int kTable = 1 << kHashLog;      // entries: position + 1, 0 = empty
constexpr uint32_t kMaxOffset = 65535;
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kLastLiterals = 5;      // the last bytes of a block are literals
constexpr uint32_t kMatchFreeTail = 12;    // no match starts within the last bytes
constexpr uint32_t kMinSplitPlane = 128;   // c-blosc splits a block when blocksize / typesize >= 128
constexpr int kStreamsPerBlock = kSlotsPerBlock;  // planes of a split block: one slot each

DSX_ZHD inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashLog); }

// may position p match at its candidate `cand` (a table entry: position + 1, 0 = none): strictly below p, in offset reach
DSX_ZHD inline bool in_reach(uint32_t cand, uint32_t p) { return cand != 0 && cand - 1 < p && p - (cand - 1) <= kMaxOffset; }

// bytes of the length chain of a field holding `len` (len = literal length, or match length - 4)
DSX_ZHD inline uint32_t chain_bytes(uint32_t len) { return len >= 15 ? (len - 15) / 255 + 1 : 0; }
// bytes of a sequence of `lit` literals and a match of `ml` bytes; of the last literals
DSX_ZHD inline uint32_t sequence_bytes(uint32_t lit, uint32_t ml) {
  return 1 + chain_bytes(lit) + lit + 2 + chain_bytes(ml - kMinMatch);
}
DSX_ZHD inline uint32_t last_bytes(uint32_t lit) { return 1 + chain_bytes(lit) + lit; }
// chain byte i of chain_bytes(len)
DSX_ZHD inline uint8_t chain_byte(uint32_t len, uint32_t i) {
  return i + 1 < chain_bytes(len) ? 255 : (uint8_t)((len - 15) % 255);
}
DSX_ZHD inline uint8_t token(uint32_t lit, uint32_t ml4) {
  return (uint8_t)(((lit < 15 ? lit : 15u) << 4) | (ml4 < 15 ? ml4 : 15u));
}

// ---- container ----------------------------------------------------------------------------------------------------
// streams of Blosc block b of a chunk of n bytes: 2 planes of bsize / 2 bytes, or the shuffled block as one stream
DSX_ZHD inline bool block_splits(const Geometry& g, uint64_t n, int b) {
  return g.bsize(n, b) == g.blocksize && g.blocksize / 2 >= kMinSplitPlane;
}
// The container of the LZ4 mode (dsx_blosc_frame.h): split streams.  Stream j is slot j as it is, sizes[j] bytes (a
// stored stream has its own length; the second entry of an unsplit block is not read); the one stream of an unsplit
// block runs on from slot 0 into slot 1.
struct Lz4Streams {
  static constexpr unsigned kFlags = kBloscShuffle | (kInnerLz4 << 5);
  static constexpr int kParts = 1;
  DSX_ZHD static int streams(const Geometry& g, uint64_t n, int b) { return block_splits(g, n, b) ? kStreamsPerBlock : 1; }
  DSX_ZHD static uint32_t stream_bytes(const uint32_t* ss, uint32_t, int j) { return ss[j]; }
  DSX_ZHD static int prefix(uint32_t, uint8_t*) { return 0; }
  DSX_ZHD static int prefix_bytes(uint32_t) { return 0; }
};

// ---- host build ---------------------------------------------------------------------------------------------------
// One stream s[0 .. n) -> out (n bytes of room); returns the bytes of the LZ4 block, 0 when the stream is stored.
// table: kTable words of work space.  Src: anything with operator[](uint32_t) -> byte.
template <class Src>
inline uint32_t encode_stream_host(const Src& s, uint32_t n, uint8_t* out, uint32_t* table) {
  auto rd4 = [&](uint32_t p) {
    return (uint32_t)s[p] | ((uint32_t)s[p + 1] << 8) | ((uint32_t)s[p + 2] << 16) | ((uint32_t)s[p + 3] << 24);
  };
  uint32_t op = 0, anchor = 0;
  if (n > kMatchFreeTail) {
    for (int i = 0; i < kTable; ++i) table[i] = 0;
    const uint32_t mstart_end = n - kMatchFreeTail, mend = n - kLastLiterals;
    uint32_t cursor = 0;
    while (cursor < mstart_end) {
      uint32_t v4[kGroup], cand[kGroup];
      int first = -1;
      for (int l = 0; l < kGroup; ++l) {
        const uint32_t p = cursor + (uint32_t)l;
        if (p >= mstart_end) { cand[l] = 0; continue; }
        v4[l] = rd4(p);
        cand[l] = table[hash4(v4[l])];
        if (first < 0 && in_reach(cand[l], p) && rd4(cand[l] - 1) == v4[l]) first = l;
      }
      for (int l = 0; l < kGroup; ++l) {
        const uint32_t p = cursor + (uint32_t)l;
        if (p >= mstart_end) break;
        uint32_t& t = table[hash4(v4[l])];
        if (t < p + 1) t = p + 1;
      }
      if (first < 0) {
        cursor += kGroup;
        if (op + ((cursor < n ? cursor : n) - anchor) >= n) return 0;
        continue;
      }
      const uint32_t start = cursor + (uint32_t)first, ref = cand[first] - 1;
      uint32_t ml = kMinMatch;
      while (start + ml < mend && s[start + ml] == s[ref + ml]) ++ml;
      const uint32_t lit = start - anchor;
      if (op + sequence_bytes(lit, ml) >= n) return 0;
      out[op++] = token(lit, ml - kMinMatch);
      for (uint32_t i = 0, k = chain_bytes(lit); i < k; ++i) out[op++] = chain_byte(lit, i);
      for (uint32_t i = 0; i < lit; ++i) out[op++] = s[anchor + i];
      put_le(out + op, start - ref, 2);
      op += 2;
      for (uint32_t i = 0, k = chain_bytes(ml - kMinMatch); i < k; ++i) out[op++] = chain_byte(ml - kMinMatch, i);
      anchor = cursor = start + ml;
    }
  }
  const uint32_t lit = n - anchor;
  if (op + last_bytes(lit) >= n) return 0;
  out[op++] = token(lit, 0);
  for (uint32_t i = 0, k = chain_bytes(lit); i < k; ++i) out[op++] = chain_byte(lit, i);
  for (uint32_t i = 0; i < lit; ++i) out[op++] = s[anchor + i];
  return op;
}

// Work space of the host build
struct HostWork {
  uint32_t table[kTable];
  uint8_t lit[kBloscBlock];                      // the shuffled block
  uint8_t slots[kSlotsPerBlock * kSlotStride];   // its encoded streams
};

// The ns streams of the shuffled block lit[0 .. bsize) -> its slots and sizes (the encode_block of assemble_chunk_host)
struct BlockEncoderHost {
  uint32_t* table;
  void operator()(const uint8_t* lit, uint32_t bsize, int ns, uint8_t* slots, uint32_t* ss) const {
    const uint32_t sn = bsize / (uint32_t)ns;
    for (int j = 0; j < ns; ++j) {
      const uint32_t coded = encode_stream_host(lit + (size_t)j * sn, sn, slots + (size_t)j * kSlotStride, table);
      ss[j] = coded ? coded : sn;
    }
  }
};

// One chunk of n bytes (uint16, n even) -> out (n + 16 bytes of room); returns the frame's bytes.
inline uint64_t encode_chunk_host(HostWork& w, const uint16_t* e, uint64_t n, int clevel, uint8_t* out) {
  return assemble_chunk_host<Lz4Streams>(e, n, clevel, w.lit, w.slots, out, BlockEncoderHost{w.table});
}

// n_chunks chunks of chunk_bytes (uint16) -> packed frames + offsets[n_chunks + 1] (the device encoder's output).
// frames: n_chunks * (chunk_bytes + 16) bytes at most.
inline void blosc_encode_host(const uint16_t* src, uint64_t n_chunks, uint64_t chunk_bytes, int clevel, uint8_t* frames,
                              int64_t* offsets) {
  uint32_t* table = new uint32_t[kTable];
  assemble_chunks_host<Lz4Streams>(src, n_chunks, chunk_bytes, clevel, frames, offsets, BlockEncoderHost{table});
  delete[] table;
}

}  // namespace lz4enc
}  // namespace dsx

#endif  // DSX_LZ4_ENC_H
