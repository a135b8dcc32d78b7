// dsx_blosc_frame.h -- the Blosc 1 container of every writer here: the constants of the format (used by the readers of
// dsx_io.h too), the geometry of a typesize-2 chunk, the frame header, and the frame of one chunk assembled from the
// encoded pieces of its blocks -- once for the host builds (assemble_chunk_host) and, over the same policy type, once
// for the device (the pack kernels of dsx_zenc_kernels.h).  Plain C++ for g++ and hipcc.
//
// Frame (c-blosc README_HEADER.rst, blosc.c): 16-byte header, one int32 start per block, then per block its streams,
// each an int32 length and the bytes; a stream as long as its share of the block is stored (the shuffled bytes).  A
// chunk under kBloscMinBuffer bytes, clevel 0, or a frame not smaller than its data is a memcpyed frame: the header
// and the chunk's bytes.
//
// An encoder leaves every Blosc block kSlotsPerBlock slots of kSlotStride bytes and as many sizes.  What a stream is
// made of is the container's business, a type C with static members only (zenc::ZstdFrames, lz4enc::Lz4Streams):
//   C::kFlags                     header flags without the memcpyed bit
//   C::kParts                     stream j is the slots j .. j + kParts - 1, sizes[] bytes of each, back to back
//   C::streams(g, n, b)           streams of block b of a chunk of n bytes
//   C::stream_bytes(sizes, sn, j) length of stream j of a block whose streams cover sn bytes each; sn = stored
//   C::prefix(sn, out)            writes what stands in front of the parts of a coded stream; returns its bytes
//   C::prefix_bytes(sn)           those bytes
#ifndef DSX_BLOSC_FRAME_H
#define DSX_BLOSC_FRAME_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef DSX_ZHD
#if defined(__HIP__) || defined(__CUDACC__)
#define DSX_ZHD __host__ __device__
#else
#define DSX_ZHD
#endif
#endif

namespace dsx {
namespace blosc {

constexpr int kBloscHeader = 16;
constexpr int kBloscMinBuffer = 128;            // shorter buffers are stored (c-blosc MIN_BUFFERSIZE)
constexpr int kBloscMaxSplits = 16;
constexpr int kBloscBlock = 256 * 1024;         // Blosc block of the writers
constexpr unsigned kBloscShuffle = 0x1, kBloscMemcpyed = 0x2, kBloscBitshuffle = 0x4, kBloscDontSplit = 0x10;
enum BloscInner { kInnerBlosclz = 0, kInnerLz4 = 1, kInnerSnappy = 2, kInnerZlib = 3, kInnerZstd = 4 };  // flags >> 5
constexpr int kSlotsPerBlock = 2;               // encoded pieces of a Blosc block: zstd blocks, or byte planes
constexpr int kSlotStride = kBloscBlock / kSlotsPerBlock + 16;  // one piece (a zstd block: 3-byte header + <= 128 KiB)

DSX_ZHD inline void put_le(uint8_t* p, uint64_t v, int n) {
  for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// Blosc geometry of one chunk of n bytes (n even)
struct Geometry {
  uint32_t blocksize;  // 256 KiB or the whole chunk
  int nblocks;         // Blosc blocks
  DSX_ZHD Geometry(uint64_t n) {
    blocksize = (uint32_t)(n < (uint64_t)kBloscBlock ? n : (uint64_t)kBloscBlock);
    nblocks = blocksize ? (int)((n + blocksize - 1) / blocksize) : 0;
  }
  DSX_ZHD uint32_t bsize(uint64_t n, int b) const {
    const uint64_t left = n - (uint64_t)b * blocksize;
    return (uint32_t)(left < blocksize ? left : blocksize);
  }
};

// byte p of a byte-shuffled typesize-2 Blosc block of `ne` elements starting at `e`
DSX_ZHD inline uint8_t shuffled_byte(const uint16_t* e, uint32_t ne, uint32_t p) {
  return p < ne ? (uint8_t)(e[p] & 255u) : (uint8_t)(e[p - ne] >> 8);
}

// flags: shuffle, "don't split" and the inner codec (<< 5); the memcpyed bit is set here
DSX_ZHD inline void blosc_header(uint8_t* out, unsigned flags, int typesize, uint64_t n, uint64_t blocksize,
                                 uint64_t cbytes, bool memcpyed) {
  out[0] = 2;  // version
  out[1] = 1;  // version of the inner codec's format
  out[2] = (uint8_t)(flags | (memcpyed ? kBloscMemcpyed : 0u));
  out[3] = (uint8_t)typesize;
  put_le(out + 4, n, 4);
  put_le(out + 8, memcpyed ? n : blocksize, 4);
  put_le(out + 12, cbytes, 4);
}

// Bytes block b takes in the frame (its streams and their lengths) from the sizes of its slots
template <class C>
DSX_ZHD inline uint64_t block_bytes(const Geometry& g, uint64_t n, int b, const uint32_t* sizes) {
  const int ns = C::streams(g, n, b);
  const uint32_t sn = g.bsize(n, b) / (uint32_t)ns;
  uint64_t f = 0;
  for (int j = 0; j < ns; ++j) f += 4 + C::stream_bytes(sizes, sn, j);
  return f;
}

// Frame bytes of one chunk (n bytes) from the sizes of its slots, sizes[nblocks][kSlotsPerBlock]; store = the chunk is
// stored as a whole (short chunk or clevel <= 0).
template <class C>
DSX_ZHD inline uint64_t chunk_frame_bytes(const uint32_t* sizes, uint64_t n, bool store) {
  if (store) return kBloscHeader + n;
  const Geometry g(n);
  uint64_t f = kBloscHeader + 4ull * g.nblocks;
  for (int b = 0; b < g.nblocks; ++b) f += block_bytes<C>(g, n, b, sizes + b * kSlotsPerBlock);
  return f < kBloscHeader + n ? f : kBloscHeader + n;  // not smaller than the data: memcpyed frame
}

// ---- host build -----------------------------------------------------------------------------------------------
// One chunk of n bytes (uint16, n even) -> out (n + 16 bytes of room); returns the frame's bytes.
// encode_block(lit, bsize, ns, slots, sizes): the shuffled block lit[0 .. bsize) of ns streams -> its slots and sizes
// (sizes arrive zeroed).  lit: kBloscBlock bytes of work space, slots: kSlotsPerBlock * kSlotStride.
// The frame turns memcpyed as soon as the position reaches the chunk's bytes -- the position only grows, so this is
// the decision chunk_frame_bytes takes from the sum --, which spares noise the encoding of its remaining blocks.
template <class C, class EncodeBlock>
inline uint64_t assemble_chunk_host(const uint16_t* e, uint64_t n, int clevel, uint8_t* lit, uint8_t* slots,
                                    uint8_t* out, EncodeBlock&& encode_block) {
  const Geometry g(n);
  uint64_t pos = kBloscHeader + 4ull * g.nblocks;
  bool memcpyed = n < (uint64_t)kBloscMinBuffer || clevel <= 0;
  for (int b = 0; b < g.nblocks && !memcpyed; ++b) {
    const uint32_t bsize = g.bsize(n, b);
    for (uint32_t p = 0; p < bsize; ++p) lit[p] = shuffled_byte(e + (uint64_t)b * (g.blocksize / 2), bsize / 2, p);
    const int ns = C::streams(g, n, b);
    const uint32_t sn = bsize / (uint32_t)ns;
    uint32_t sizes[kSlotsPerBlock] = {};
    encode_block((const uint8_t*)lit, bsize, ns, slots, sizes);
    put_le(out + kBloscHeader + 4 * b, pos, 4);
    for (int j = 0; j < ns; ++j) {
      const uint32_t m = C::stream_bytes(sizes, sn, j);
      if (pos + 4 + m >= kBloscHeader + n) { memcpyed = true; break; }
      put_le(out + pos, m, 4);
      uint8_t* d = out + pos + 4;
      if (m == sn) {
        memcpy(d, lit + (size_t)j * sn, sn);
      } else {
        d += C::prefix(sn, d);
        for (int k = j; k < j + C::kParts; ++k) {
          memcpy(d, slots + (size_t)k * kSlotStride, sizes[k]);
          d += sizes[k];
        }
      }
      pos += 4 + m;
    }
  }
  if (memcpyed) {
    if (n) memcpy(out + kBloscHeader, e, n);
    pos = kBloscHeader + n;
  }
  blosc_header(out, C::kFlags, 2, n, g.blocksize, pos, memcpyed);
  return pos;
}

// n_chunks chunks of chunk_bytes (uint16) -> packed frames + offsets[n_chunks + 1] (the device encoder's output).
// frames: n_chunks * (chunk_bytes + 16) bytes at most.
template <class C, class EncodeBlock>
inline void assemble_chunks_host(const uint16_t* src, uint64_t n_chunks, uint64_t chunk_bytes, int clevel,
                                 uint8_t* frames, int64_t* offsets, EncodeBlock&& encode_block) {
  uint8_t* work = new uint8_t[kBloscBlock + (size_t)kSlotsPerBlock * kSlotStride];
  uint64_t at = 0;
  offsets[0] = 0;
  for (uint64_t c = 0; c < n_chunks; ++c) {
    at += assemble_chunk_host<C>(src + c * (chunk_bytes / 2), chunk_bytes, clevel, work, work + kBloscBlock, frames + at,
                                 encode_block);
    offsets[c + 1] = (int64_t)at;
  }
  delete[] work;
}

}  // namespace blosc
}  // namespace dsx

#endif  // DSX_BLOSC_FRAME_H
