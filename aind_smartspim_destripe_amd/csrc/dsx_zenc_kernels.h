// dsx_zenc_kernels.h -- Blosc-zstd frames on the device (dsx_blosc_encode_device): the encoder core of dsx_zstd_enc.h
// run by one workgroup per zstd block, then a size scan and a copy into one packed buffer.
//
//   k_zenc_block   grid = chunks x Blosc blocks x 2: wave k reads literal stream k of the block (the byte shuffle
//                  is done on the load) into an LDS histogram; thread 0 builds the code (dsx_zstd_enc.h plan_block);
//                  wave k then packs stream k: per round 64 lanes x 8 literals, bit offsets from a wave prefix sum of
//                  the code lengths, codes OR-ed into an LDS word window, full words stored, the partial word carried.
//                  Each block lands in a slot of kSlotStride bytes; its size in sizes[].
//   k_zenc_scan    one workgroup: frame bytes per chunk (chunk_frame_bytes) and their exclusive scan -> offsets.
//   k_zenc_copy    grid = chunks x Blosc blocks: block table entry, stream length and stream (zstd frame header + the
//                  slots, or the stored shuffled block), or the chunk's bytes of a memcpyed frame.
#ifndef DSX_ZENC_KERNELS_H
#define DSX_ZENC_KERNELS_H

#include <hip/hip_runtime.h>

#include "dsx_zstd_enc.h"

namespace dsx {
namespace zenc {

constexpr int kEncThreads = 256;  // 4 waves: one per literal stream
constexpr int kLitPerLane = 8;
constexpr int kRound = 64 * kLitPerLane;
constexpr int kWinWords = (kRound * kMaxBits) / 32 + 2;  // bit window of one round + the carried word

struct EncArgs {
  const uint16_t* src;  // n_chunks chunks of chunk_bytes
  uint8_t* slots;       // [n_chunks][nblocks][kZPerBlosc] x kSlotStride
  uint32_t* sizes;      // [n_chunks][nblocks][kZPerBlosc]
  uint64_t chunk_bytes;
  int nblocks;
};

__global__ void __launch_bounds__(kEncThreads) k_zenc_block(EncArgs a) {
  __shared__ HufWork h;
  __shared__ uint32_t win[4][kWinWords];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t zb = blockIdx.x % (uint32_t)(a.nblocks * kZPerBlosc);
  const uint64_t chunk = blockIdx.x / (uint32_t)(a.nblocks * kZPerBlosc);
  const int b = (int)(zb / kZPerBlosc), j = (int)(zb % kZPerBlosc);
  const Geometry g(a.chunk_bytes);
  const uint32_t bsize = g.bsize(a.chunk_bytes, b);
  const uint32_t z0 = (uint32_t)j * kZBlock;
  if (z0 >= bsize) {
    if (tid == 0) a.sizes[blockIdx.x] = 0;
    return;
  }
  const int n = (int)((bsize - z0) < (uint32_t)kZBlock ? bsize - z0 : (uint32_t)kZBlock);
  const bool last = z0 + (uint32_t)n == bsize;
  const uint16_t* e = a.src + chunk * (a.chunk_bytes / 2) + (uint64_t)b * (g.blocksize / 2);
  const uint32_t ne = bsize / 2;
  uint8_t* slot = a.slots + (uint64_t)blockIdx.x * kSlotStride;

  for (int i = tid; i < 4 * 256; i += kEncThreads) (&h.scount[0][0])[i] = 0;
  __syncthreads();
  const int s0 = stream_begin(n, wave), s1 = stream_begin(n, wave + 1);
  for (int i = s0 + lane; i < s1; i += 64) atomicAdd(&h.scount[wave][shuffled_byte(e, ne, z0 + i)], 1u);
  __syncthreads();
  {
    const int s = tid;
    h.count[s] = h.scount[0][s] + h.scount[1][s] + h.scount[2][s] + h.scount[3][s];
  }
  __syncthreads();
  {
    const int s = tid;
    if (h.count[s]) h.sorted[sort_rank(h, s)] = sort_key(h, s);
    const int present = __syncthreads_count(h.count[s] != 0);
    if (tid == 0) {
      h.nsym = present;
      plan_block(h, n);
      write_block_frame(h, n, last, slot);
      a.sizes[blockIdx.x] = (uint32_t)h.block_bytes;
    }
  }
  __syncthreads();
  if (h.type == kRaw) {
    for (int i = tid; i < n; i += kEncThreads) slot[3 + i] = shuffled_byte(e, ne, z0 + i);
    return;
  }
  if (h.type != kCompressed) return;

  // ---- stream `wave`: literals s1 - 1 down to s0, rounds of 64 x 8 (equal round count in every wave: __syncthreads)
  uint8_t* dst = slot + h.prefix_bytes;
  for (int k = 0; k < wave; ++k) dst += h.stream_bytes[k];
  const int rounds = (stream_begin(n, 1) + kRound - 1) / kRound;
  uint32_t* w = win[wave];
  for (int q = lane; q < kWinWords; q += 64) w[q] = 0;
  uint32_t bitpos = 0;  // bits of this stream written so far (uniform in the wave)
  __syncthreads();
  for (int r = 0; r < rounds; ++r) {
    const int rev0 = r * kRound + lane * kLitPerLane;  // reversed index of this lane's first literal
    uint32_t codes[kLitPerLane];
    int lens[kLitPerLane];
    int mine = 0;
#pragma unroll
    for (int t = 0; t < kLitPerLane; ++t) {
      const int i = s1 - 1 - (rev0 + t);
      if (i >= s0) {
        const uint8_t v = shuffled_byte(e, ne, z0 + i);
        codes[t] = h.code[v];
        lens[t] = h.len[v];
      } else {
        codes[t] = 0;
        lens[t] = 0;
      }
      mine += lens[t];
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    const int total = __shfl(incl, 63, 64);
    int off = (int)(bitpos & 31u) + incl - mine;
#pragma unroll
    for (int t = 0; t < kLitPerLane; ++t) {
      if (lens[t]) {
        const int q = off >> 5, sh = off & 31;
        atomicOr(&w[q], codes[t] << sh);
        if (sh + lens[t] > 32) atomicOr(&w[q + 1], codes[t] >> (32 - sh));
        off += lens[t];
      }
    }
    __syncthreads();
    const int nfull = ((int)(bitpos & 31u) + total) >> 5;
    uint8_t* wd = dst + 4 * (bitpos >> 5);
    for (int q = lane; q < nfull; q += 64) {
      const uint32_t v = w[q];
      wd[4 * q] = (uint8_t)v; wd[4 * q + 1] = (uint8_t)(v >> 8); wd[4 * q + 2] = (uint8_t)(v >> 16);
      wd[4 * q + 3] = (uint8_t)(v >> 24);
    }
    const uint32_t carry = w[nfull];
    __syncthreads();
    for (int q = lane; q <= nfull; q += 64) w[q] = (q == 0) ? carry : 0u;
    bitpos += (uint32_t)total;
    __syncthreads();
  }
  if (lane == 0) {  // end mark, then the bytes of the partial word
    const uint32_t v = w[0] | (1u << (bitpos & 31u));
    const int rest = (int)h.stream_bytes[wave] - 4 * (int)(bitpos >> 5);
    uint8_t* wd = dst + 4 * (bitpos >> 5);
    for (int i = 0; i < rest; ++i) wd[i] = (uint8_t)(v >> (8 * i));
  }
}

struct PackArgs {
  const uint16_t* src;
  const uint8_t* slots;
  const uint32_t* sizes;
  uint8_t* frames;
  int64_t* offsets;  // [n_chunks + 1]
  uint64_t chunk_bytes;
  int n_chunks, nblocks;
  bool store;        // every chunk is a memcpyed frame (short chunks, clevel <= 0)
};

__global__ void __launch_bounds__(256) k_zenc_scan(PackArgs a) {
  __shared__ int64_t part[256];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; a.offsets[0] = 0; }
  __syncthreads();
  const int per = a.nblocks * kZPerBlosc;
  for (int c0 = 0; c0 < a.n_chunks; c0 += 256) {
    const int c = c0 + tid;
    int64_t v = c < a.n_chunks ? (int64_t)chunk_frame_bytes(a.sizes + (uint64_t)c * per, a.chunk_bytes, a.store) : 0;
    part[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t o = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += o;
      __syncthreads();
    }
    if (c < a.n_chunks) a.offsets[c + 1] = carry + part[tid];
    __syncthreads();
    if (tid == 255) carry += part[255];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_zenc_copy(PackArgs a) {
  const int tid = threadIdx.x;
  const uint64_t chunk = blockIdx.x / (uint32_t)a.nblocks;
  const int b = (int)(blockIdx.x % (uint32_t)a.nblocks);
  const uint64_t n = a.chunk_bytes;
  const Geometry g(n);
  uint8_t* out = a.frames + a.offsets[chunk];
  const uint64_t fbytes = (uint64_t)(a.offsets[chunk + 1] - a.offsets[chunk]);
  const bool memcpyed = fbytes >= kBloscHeader + n;
  if (b == 0 && tid == 0) blosc_header(out, n, g.blocksize, fbytes, memcpyed);
  const uint8_t* raw = (const uint8_t*)(a.src + chunk * (n / 2));
  const uint32_t bsize = a.store ? (uint32_t)n : g.bsize(n, b);
  if (memcpyed) {
    const uint64_t o = (uint64_t)b * g.blocksize;
    if (a.store && b > 0) return;
    for (uint32_t i = tid; i < bsize; i += 256) out[kBloscHeader + o + i] = raw[o + i];
    return;
  }
  const uint32_t* zs_chunk = a.sizes + chunk * (uint64_t)(a.nblocks * kZPerBlosc);
  uint64_t pos = kBloscHeader + 4ull * g.nblocks;
  for (int k = 0; k < b; ++k) pos += 4 + blosc_stream_bytes(zs_chunk + k * kZPerBlosc, g.bsize(n, k));
  const uint32_t* zs = zs_chunk + b * kZPerBlosc;
  const uint32_t sb = blosc_stream_bytes(zs, bsize);
  uint8_t* d = out + pos + 4;
  if (tid == 0) {
    put_le(out + kBloscHeader + 4 * b, pos, 4);
    put_le(out + pos, sb, 4);
  }
  if (sb == bsize) {  // stored stream: the shuffled block
    const uint16_t* e = a.src + chunk * (n / 2) + (uint64_t)b * (g.blocksize / 2);
    for (uint32_t p = tid; p < bsize; p += 256) d[p] = shuffled_byte(e, bsize / 2, p);
    return;
  }
  const int fh = frame_header_bytes(bsize);
  if (tid == 0) frame_header(bsize, d);
  d += fh;
  for (int j = 0; j < kZPerBlosc; ++j) {
    const uint32_t* sl = (const uint32_t*)(a.slots + ((uint64_t)blockIdx.x * kZPerBlosc + j) * kSlotStride);
    const uint32_t m = zs[j];
    for (uint32_t q = tid; 4 * q < m; q += 256) {
      const uint32_t v = sl[q];
      const uint32_t i = 4 * q;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (i + t < m) d[i + t] = (uint8_t)(v >> (8 * t));
    }
    d += m;
  }
}

}  // namespace zenc
}  // namespace dsx

#endif  // DSX_ZENC_KERNELS_H
