// dsx_lz4enc_kernels.h -- Blosc-LZ4 frames on the device (dsx_blosc_encode_device_ex, DSX_ZENC_LZ4): the finder of
// dsx_lz4_enc.h run by one wave per stream; the pack stage of dsx_zenc_kernels.h (k_pack_scan / k_pack_copy over
// Lz4Streams) then makes the frames.
//
//   k_lz4_stream   grid = chunks x Blosc blocks x 2, one wave each: stream j of the block (plane j of a split block;
//                  the whole shuffled block for j = 0 of an unsplit one, whose j = 1 leaves at once).  Serial over the
//                  sequences, 64 lanes wide inside a step: lane l hashes position cursor + l (the byte shuffle is done
//                  on the load) and looks its candidate up in the LDS table, then every lane enters its position with
//                  an LDS atomicMax (the highest position wins: no racing store); the first verified lane is taken
//                  with a ballot; the match is extended 64 x 8 bytes per round (shuffled_word, a ballot on the first
//                  mismatch); the literals are copied by the whole wave; token and offset are written by one lane.
//                  All match reads go to the source, the output is never read back.  cursor, anchor and the output
//                  position are wave-uniform.  The stream lands in its slot (kSlotStride bytes; an unsplit block of up
//                  to 256 KiB - 2 bytes runs on into the slot of its idle j = 1), its length in sizes[] (the stream's
//                  own length = stored: nothing in the slot is read then).
#ifndef DSX_LZ4ENC_KERNELS_H
#define DSX_LZ4ENC_KERNELS_H

#include <hip/hip_runtime.h>

#include "dsx_lz4_enc.h"
#include "dsx_zenc_kernels.h"  // EncArgs, shuffled_word

namespace dsx {
namespace lz4enc {

static_assert(kGroup == 64, "one position per lane");

__global__ void __launch_bounds__(64) k_lz4_stream(zenc::EncArgs a) {
  __shared__ uint32_t table[kTable];
  const uint32_t lane = threadIdx.x;
  const uint32_t sb = blockIdx.x % (uint32_t)(a.nblocks * kStreamsPerBlock);
  const uint64_t chunk = blockIdx.x / (uint32_t)(a.nblocks * kStreamsPerBlock);
  const int b = (int)(sb / kStreamsPerBlock), j = (int)(sb % kStreamsPerBlock);
  const Geometry g(a.chunk_bytes);
  const uint32_t bsize = g.bsize(a.chunk_bytes, b);
  const bool split = block_splits(g, a.chunk_bytes, b);
  if (!split && j) {
    if (lane == 0) a.sizes[blockIdx.x] = 0;
    return;
  }
  const uint16_t* e = a.src + chunk * (a.chunk_bytes / 2) + (uint64_t)b * (g.blocksize / 2);
  const uint32_t ne = bsize / 2;
  const uint32_t n = split ? ne : bsize;   // bytes of the stream
  const uint32_t s0 = (uint32_t)j * ne;    // its first byte in the shuffled block; it ends at s0 + n
  uint8_t* out = a.slots + (uint64_t)blockIdx.x * kSlotStride;
  auto rd4 = [&](uint32_t p) {
    return (uint32_t)shuffled_byte(e, ne, s0 + p) | ((uint32_t)shuffled_byte(e, ne, s0 + p + 1) << 8) |
           ((uint32_t)shuffled_byte(e, ne, s0 + p + 2) << 16) | ((uint32_t)shuffled_byte(e, ne, s0 + p + 3) << 24);
  };
  uint32_t op = 0, anchor = 0;
  bool stored = false;
  if (n > kMatchFreeTail) {
    for (int i = (int)lane; i < kTable; i += 64) table[i] = 0;
    __syncthreads();
    const uint32_t mstart_end = n - kMatchFreeTail, mend = n - kLastLiterals;
    uint32_t cursor = 0;
    while (cursor < mstart_end) {
      const uint32_t p = cursor + lane;
      const bool valid = p < mstart_end;
      uint32_t v4 = 0, h = 0, cand = 0;
      if (valid) {
        v4 = rd4(p);
        h = hash4(v4);
        cand = table[h];
      }
      const bool ok = valid && in_reach(cand, p) && rd4(cand - 1) == v4;
      __syncthreads();  // every look-up of the group before its entries
      if (valid) atomicMax(&table[h], p + 1);
      __syncthreads();
      const unsigned long long found = __ballot(ok);
      if (!found) {
        cursor += kGroup;
        if (op + ((cursor < n ? cursor : n) - anchor) >= n) { stored = true; break; }
        continue;
      }
      const int first = __ffsll((long long)found) - 1;
      const uint32_t start = cursor + (uint32_t)first, ref = (uint32_t)__shfl((int)cand, first, 64) - 1;
      // ---- extend: rounds of 64 x 8 bytes, none at or behind mend
      uint32_t ml = kMinMatch;
      for (;;) {
        const uint32_t q = start + ml + 8 * lane;  // this lane's 8 bytes
        const uint32_t room = q < mend ? (mend - q < 8u ? mend - q : 8u) : 0u;
        uint32_t same = 0;
        if (room) {
          const uint64_t x = zenc::shuffled_word(e, ne, s0 + q, s0 + q + room) ^
                             zenc::shuffled_word(e, ne, s0 + q - (start - ref), s0 + q - (start - ref) + room);
          same = x ? (uint32_t)(__ffsll((long long)x) - 1) >> 3 : 8u;
          if (same > room) same = room;
        }
        const unsigned long long stop = __ballot(same < 8u);
        if (!stop) { ml += 8 * 64; continue; }
        const int at = __ffsll((long long)stop) - 1;
        ml += 8 * (uint32_t)at + (uint32_t)__shfl((int)same, at, 64);
        break;
      }
      const uint32_t lit = start - anchor;
      if (op + sequence_bytes(lit, ml) >= n) { stored = true; break; }
      const uint32_t kl = chain_bytes(lit), km = chain_bytes(ml - kMinMatch);
      uint8_t* d = out + op;
      if (lane == 0) d[0] = token(lit, ml - kMinMatch);
      for (uint32_t i = lane; i < kl; i += 64) d[1 + i] = chain_byte(lit, i);
      d += 1 + kl;
      for (uint32_t i = lane; i < lit; i += 64) d[i] = shuffled_byte(e, ne, s0 + anchor + i);
      d += lit;
      if (lane == 0) {
        d[0] = (uint8_t)(start - ref);
        d[1] = (uint8_t)((start - ref) >> 8);
      }
      for (uint32_t i = lane; i < km; i += 64) d[2 + i] = chain_byte(ml - kMinMatch, i);
      op += sequence_bytes(lit, ml);
      anchor = cursor = start + ml;
    }
  }
  const uint32_t lit = n - anchor;
  if (!stored && op + last_bytes(lit) >= n) stored = true;
  if (stored) {
    if (lane == 0) a.sizes[blockIdx.x] = n;
    return;
  }
  const uint32_t kl = chain_bytes(lit);
  uint8_t* d = out + op;
  if (lane == 0) {
    d[0] = token(lit, 0);
    a.sizes[blockIdx.x] = op + last_bytes(lit);
  }
  for (uint32_t i = lane; i < kl; i += 64) d[1 + i] = chain_byte(lit, i);
  d += 1 + kl;
  for (uint32_t i = lane; i < lit; i += 64) d[i] = shuffled_byte(e, ne, s0 + anchor + i);
}

}  // namespace lz4enc
}  // namespace dsx

#endif  // DSX_LZ4ENC_KERNELS_H
