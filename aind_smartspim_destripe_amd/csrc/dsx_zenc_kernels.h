// dsx_zenc_kernels.h -- Blosc-zstd frames on the device (dsx_blosc_encode_device): the encoder core of dsx_zstd_enc.h
// run by one workgroup per zstd block, then a size scan and a copy into one packed buffer.
//
//   k_zenc_block   grid = chunks x Blosc blocks x 2: wave k reads literal stream k of the block (the byte shuffle
//                  is done on the load) into an LDS histogram; thread 0 builds the code (dsx_zstd_enc.h plan_block);
//                  wave k then packs stream k: per round 64 lanes x 8 literals, bit offsets from a wave prefix sum of
//                  the code lengths, codes OR-ed into an LDS word window, full words stored, the partial word carried.
//                  Each block lands in a slot of kSlotStride bytes; its size in sizes[].
//   k_zenc_block_runs  the same grid in runs mode (dsx_zstd_enc.h kModeRuns).  Thread t owns the contiguous piece
//                  [t * P, (t + 1) * P) of the block (8 shuffled bytes per 16-byte load).  Pass 1 walks the piece as
//                  stretches of equal bytes: the entropy-only histogram (one LDS atomic per stretch and stream), the
//                  first and the last run start of the piece, the qualifying runs inside it; the neighbours' run
//                  starts give the run that enters the piece and the end of the one that leaves it.  A workgroup scan
//                  numbers the qualifying runs (the first kSeqCap are kept), a second walk counts the literals that
//                  remain, a scan gives every piece its literal index, a third walk compacts the literals into the
//                  block's work buffer, counts them per literal stream and writes the sequence list.  Then three
//                  threads work side by side: the entropy-only plan, the plan of the literals section, the sequences
//                  bit stream (behind the compacted literals); the smaller block is written, its streams packed by
//                  the same pack_streams, from the source or from the compacted literals.  A block without a run of
//                  kMinRun bytes, or of one value, leaves after pass 1 and is written as k_zenc_block writes it
//                  (write_entropy_block).
// The pack stage is the same for every encoder that fills slots and sizes (k_lz4_stream of dsx_lz4enc_kernels.h too),
// templated on the container C of dsx_blosc_frame.h (ZstdFrames here, lz4enc::Lz4Streams):
//   k_pack_scan<C> one workgroup: frame bytes per chunk (chunk_frame_bytes<C>) and their exclusive scan -> offsets.
//   k_pack_copy<C> grid = chunks x Blosc blocks: block table entry, then per stream its length and its bytes (C's prefix
//                  + the slots, or the stored shuffled bytes), or the chunk's bytes of a memcpyed frame.
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

// The zstd block of workgroup blockIdx.x: block j of Blosc block b of a chunk
struct ZBlock {
  uint64_t chunk;
  int b, j;
  uint32_t bsize, z0;  // bytes of the Blosc block; first byte of the zstd block in it
  int n;               // bytes of the zstd block
  bool last;           // the last zstd block of its frame
  const uint16_t* e;   // elements of the Blosc block
  uint32_t ne;
  uint8_t* slot;
  // false: the slot lies beyond the Blosc block -- its size is written as 0 and the workgroup leaves
  __device__ __forceinline__ bool locate(const EncArgs& a) {
    const uint32_t zb = blockIdx.x % (uint32_t)(a.nblocks * kZPerBlosc);
    chunk = blockIdx.x / (uint32_t)(a.nblocks * kZPerBlosc);
    b = (int)(zb / kZPerBlosc);
    j = (int)(zb % kZPerBlosc);
    const Geometry g(a.chunk_bytes);
    bsize = g.bsize(a.chunk_bytes, b);
    z0 = (uint32_t)j * kZBlock;
    if (z0 >= bsize) {
      if (threadIdx.x == 0) a.sizes[blockIdx.x] = 0;
      return false;
    }
    n = (int)((bsize - z0) < (uint32_t)kZBlock ? bsize - z0 : (uint32_t)kZBlock);
    last = z0 + (uint32_t)n == bsize;
    e = a.src + chunk * (a.chunk_bytes / 2) + (uint64_t)b * (g.blocksize / 2);
    ne = bsize / 2;
    slot = a.slots + (uint64_t)blockIdx.x * kSlotStride;
    return true;
  }
};

// count[] and sorted[] of h from its stream histograms; returns the symbols present (every thread)
__device__ inline int finish_counts(HufWork& h) {
  const int s = threadIdx.x;
  h.count[s] = h.scount[0][s] + h.scount[1][s] + h.scount[2][s] + h.scount[3][s];
  __syncthreads();
  if (h.count[s]) h.sorted[sort_rank(h, s)] = sort_key(h, s);
  return __syncthreads_count(h.count[s] != 0);
}

// The four Huffman streams of nlit literals lit(i) -> dst, wave k packs stream k: literals s1 - 1 down to s0 in rounds
// of 64 x 8 (an equal round count in every wave: __syncthreads)
template <class Lit>
__device__ inline void pack_streams(const HufWork& h, uint32_t (*win)[kWinWords], int nlit, uint8_t* dst, Lit&& lit) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s0 = stream_begin(nlit, wave), s1 = stream_begin(nlit, wave + 1);
  for (int k = 0; k < wave; ++k) dst += h.stream_bytes[k];
  const int rounds = (stream_begin(nlit, 1) + kRound - 1) / kRound;
  uint32_t* w = win[wave];
  for (int q = lane; q < kWinWords; q += 64) w[q] = 0;
  uint32_t bitpos = 0;
  __syncthreads();
  for (int r = 0; r < rounds; ++r) {
    const int rev0 = r * kRound + lane * kLitPerLane;
    uint32_t codes[kLitPerLane];
    int lens[kLitPerLane];
    int mine = 0;
#pragma unroll
    for (int t = 0; t < kLitPerLane; ++t) {
      const int i = s1 - 1 - (rev0 + t);
      if (i >= s0) {
        const uint8_t v = lit(i);
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
  if (lane == 0) {
    const uint32_t v = w[0] | (1u << (bitpos & 31u));
    const int rest = (int)h.stream_bytes[wave] - 4 * (int)(bitpos >> 5);
    uint8_t* wd = dst + 4 * (bitpos >> 5);
    for (int i = 0; i < rest; ++i) wd[i] = (uint8_t)(v >> (8 * i));
  }
}

// The entropy-only block planned in h (plan_block) -> the slot: block frame and size by thread 0, then the raw bytes
// or the four streams, read from the source
__device__ __forceinline__ void write_entropy_block(const HufWork& h, uint32_t (*win)[kWinWords], const EncArgs& a,
                                                    const ZBlock& k) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    write_block_frame(h, k.n, k.last, k.slot);
    a.sizes[blockIdx.x] = (uint32_t)h.block_bytes;
  }
  if (h.type == kRaw) {
    for (int i = tid; i < k.n; i += kEncThreads) k.slot[3 + i] = shuffled_byte(k.e, k.ne, k.z0 + i);
  } else if (h.type == kCompressed) {
    pack_streams(h, win, k.n, k.slot + h.prefix_bytes, [&](int i) { return shuffled_byte(k.e, k.ne, k.z0 + i); });
  }
}

__global__ void __launch_bounds__(kEncThreads) k_zenc_block(EncArgs a) {
  __shared__ HufWork h;
  __shared__ uint32_t win[4][kWinWords];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  ZBlock k;
  if (!k.locate(a)) return;
  for (int i = tid; i < 4 * 256; i += kEncThreads) (&h.scount[0][0])[i] = 0;
  __syncthreads();
  const int s0 = stream_begin(k.n, wave), s1 = stream_begin(k.n, wave + 1);
  for (int i = s0 + lane; i < s1; i += 64) atomicAdd(&h.scount[wave][shuffled_byte(k.e, k.ne, k.z0 + i)], 1u);
  __syncthreads();
  const int nsym = finish_counts(h);
  if (tid == 0) {
    h.nsym = nsym;
    plan_block(h, k.n);
  }
  __syncthreads();
  write_entropy_block(h, win, a, k);
}

// ---- runs mode ---------------------------------------------------------------------------------------------------
struct RunArgs {
  EncArgs e;
  uint8_t* lits;  // [n_chunks][nblocks][kZPerBlosc] x kSlotStride: compacted literals, the sequences section behind
};

constexpr uint32_t kNoRun = 0xFFFFFFFFu;

// bytes p .. p + 7 of a byte-shuffled Blosc block (shuffled_byte; byte i in bits 8 i); positions from `end` on are not
// read.  One 16-byte load when the eight bytes lie in one plane and the address allows it.
__device__ inline uint64_t shuffled_word(const uint16_t* e, uint32_t ne, uint32_t p, uint32_t end) {
  if (p + 8 <= end && (p + 8 <= ne || p >= ne)) {
    const uint16_t* q = p < ne ? e + p : e + (p - ne);
    if (((uintptr_t)q & 15) == 0) {
      const uint4 v = *(const uint4*)q;
      const int sh = p < ne ? 0 : 8;
      const uint32_t a = ((v.x >> sh) & 255u) | (((v.x >> (16 + sh)) & 255u) << 8);
      const uint32_t b = ((v.y >> sh) & 255u) | (((v.y >> (16 + sh)) & 255u) << 8);
      const uint32_t c = ((v.z >> sh) & 255u) | (((v.z >> (16 + sh)) & 255u) << 8);
      const uint32_t d = ((v.w >> sh) & 255u) | (((v.w >> (16 + sh)) & 255u) << 8);
      return (uint64_t)(a | (b << 16)) | ((uint64_t)(c | (d << 16)) << 32);
    }
  }
  uint64_t w = 0;
  for (int t = 0; t < 8; ++t)
    if (p + t < end) w |= (uint64_t)shuffled_byte(e, ne, p + t) << (8 * t);
  return w;
}

// The piece [p0, p1) of the zstd block at z0 as maximal stretches of equal bytes: f(start, end, value, flagged), in
// order; flagged = a run starts at `start` (only the first stretch of a piece may continue a run).  p0 % 8 == 0.
template <class F>
__device__ inline void walk_piece(const uint16_t* e, uint32_t ne, uint32_t z0, uint32_t p0, uint32_t p1, F&& f) {
  if (p0 >= p1) return;
  uint32_t cur = shuffled_byte(e, ne, z0 + p0);
  bool flagged = p0 == 0 || shuffled_byte(e, ne, z0 + p0 - 1) != cur;
  uint32_t s = p0;
  for (uint32_t q = p0; q < p1; q += 8) {
    const uint64_t w = shuffled_word(e, ne, z0 + q, z0 + p1);
    if (q + 8 <= p1 && w == cur * 0x0101010101010101ull) continue;
    const uint32_t m = p1 - q < 8u ? p1 - q : 8u;
    for (uint32_t t = 0; t < m; ++t) {
      const uint32_t v = (uint32_t)(w >> (8 * t)) & 255u;
      if (v != cur) {
        f(s, q + t, cur, flagged);
        s = q + t;
        cur = v;
        flagged = true;
      }
    }
  }
  f(s, p1, cur, flagged);
}

// cnt items of value v at [at, at + cnt) of n items in four streams -> sc[stream][v]
__device__ inline void count_stretch(uint32_t (*sc)[256], int n, uint32_t at, uint32_t cnt, uint32_t v) {
  const uint32_t seg = (uint32_t)(n + 3) / 4;
  for (uint32_t a = at, end = at + cnt; a < end;) {
    const uint32_t k = a / seg, b = (k + 1) * seg < end ? (k + 1) * seg : end;
    atomicAdd(&sc[k][v], b - a);
    a = b;
  }
}

// exclusive scan of v over the 256 threads (ws: 4 words of LDS); *total = the sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* ws, uint32_t* total) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  __syncthreads();  // (ws may still be read from the scan before)
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (int k = 0; k < wave; ++k) base += ws[k];
  *total = ws[0] + ws[1] + ws[2] + ws[3];
  return base + incl - v;
}

__global__ void __launch_bounds__(kEncThreads) k_zenc_block_runs(RunArgs ra) {
  __shared__ HufWork h, h2;
  __shared__ SeqWork sw;
  __shared__ uint32_t win[4][kWinWords];
  __shared__ uint32_t run_first[kEncThreads], run_last[kEncThreads], ws[4];
  const EncArgs& a = ra.e;
  const int tid = threadIdx.x;
  ZBlock k;
  if (!k.locate(a)) return;
  const int n = k.n;
  const uint32_t z0 = k.z0, ne = k.ne;
  const uint16_t* e = k.e;
  uint8_t* slot = k.slot;
  uint8_t* lits = ra.lits + (uint64_t)blockIdx.x * kSlotStride;

  for (int i = tid; i < 4 * 256; i += kEncThreads) {
    (&h.scount[0][0])[i] = 0;
    (&h2.scount[0][0])[i] = 0;
  }
  __syncthreads();
  // ---- pass 1: the entropy-only histogram, the run starts of the piece
  const uint32_t piece = (((uint32_t)n + kEncThreads - 1) / kEncThreads + 7u) & ~7u;
  const uint32_t p0 = (uint32_t)tid * piece < (uint32_t)n ? (uint32_t)tid * piece : (uint32_t)n;
  const uint32_t p1 = p0 + piece < (uint32_t)n ? p0 + piece : (uint32_t)n;
  uint32_t first = kNoRun, lastrun = kNoRun, nq = 0;
  walk_piece(e, ne, z0, p0, p1, [&](uint32_t s, uint32_t t, uint32_t v, bool flagged) {
    count_stretch(h.scount, n, s, t - s, v);
    if (flagged) {
      if (first == kNoRun) first = s;
      lastrun = s;
      if (t < p1 && t - s >= (uint32_t)kMinRun) ++nq;
    }
  });
  run_first[tid] = first;
  run_last[tid] = lastrun;
  const int changes = __syncthreads_count(tid == 0 ? lastrun != 0u : first != kNoRun);
  uint32_t prev_start = 0, next_start = (uint32_t)n, excl = 0, nq_all = 0;
  if (changes) {  // (a block of one value is an RLE block)
    for (int u = tid - 1; u >= 0; --u)
      if (run_last[u] != kNoRun) { prev_start = run_last[u]; break; }
    for (int u = tid + 1; u < kEncThreads; ++u)
      if (run_first[u] != kNoRun) { next_start = run_first[u]; break; }
    if (lastrun != kNoRun && next_start - lastrun >= (uint32_t)kMinRun) ++nq;
    excl = block_scan(nq, ws, &nq_all);
  }
  const int nsym = finish_counts(h);
  int nl = 0, nsym2 = 0;
  if (nq_all) {
    // ---- pass 2: the literals the kept runs leave in the piece; pass 3: compact them, count them, list the sequences
    uint32_t nlit_mine = 0;
    {
      uint32_t k = 0;
      walk_piece(e, ne, z0, p0, p1, [&](uint32_t s, uint32_t t, uint32_t, bool flagged) {
        const uint32_t start = flagged ? s : prev_start, end = t < p1 ? t : next_start;
        const bool q = end - start >= (uint32_t)kMinRun;
        const bool kept = q && (flagged ? excl + k : excl - 1) < (uint32_t)kSeqCap;
        if (flagged && q) ++k;
        nlit_mine += kept ? (flagged ? 1u : 0u) : t - s;
      });
    }
    uint32_t nl_all;
    uint32_t li = block_scan(nlit_mine, ws, &nl_all);
    nl = (int)nl_all;
    {
      uint32_t k = 0;
      walk_piece(e, ne, z0, p0, p1, [&](uint32_t s, uint32_t t, uint32_t v, bool flagged) {
        const uint32_t start = flagged ? s : prev_start, end = t < p1 ? t : next_start;
        const bool q = end - start >= (uint32_t)kMinRun;
        const uint32_t idx = flagged ? excl + k : excl - 1;
        const bool kept = q && idx < (uint32_t)kSeqCap;
        if (flagged && q) ++k;
        if (kept && flagged) {
          sw.pos[idx] = s;
          sw.len[idx] = end - s;
        }
        const uint32_t cnt = kept ? (flagged ? 1u : 0u) : t - s;
        if (cnt) count_stretch(h2.scount, nl, li, cnt, v);
        for (uint32_t i = 0; i < cnt; ++i) lits[li + i] = (uint8_t)v;
        li += cnt;
      });
    }
    __syncthreads();
    nsym2 = finish_counts(h2);
  }
  // ---- three plans side by side (a block without a qualifying run has the first one only)
  if (tid == 0) {
    h.nsym = nsym;
    plan_block(h, n);
  } else if (nq_all && tid == 64) {
    h2.nsym = nsym2;
    plan_literals(h2, nl);
  } else if (nq_all && tid == 128) {
    sw.nseq = (int)(nq_all < (uint32_t)kSeqCap ? nq_all : (uint32_t)kSeqCap);
    sw.seq_bytes = encode_sequences(sw, lits + nl, kSlotStride - nl);
  }
  __syncthreads();
  const int bytes1 = nq_all ? runs_block_bytes(h2, sw.seq_bytes) : 0;
  if (!nq_all || sw.seq_bytes < 0 || bytes1 >= h.block_bytes) {  // the entropy-only block is not larger: it stays
    write_entropy_block(h, win, a, k);
    return;
  }
  if (tid == 0) {
    write_runs_block_header(bytes1, k.last, slot);
    write_literals_head(h2, nl, slot + 3);
    a.sizes[blockIdx.x] = (uint32_t)bytes1;
  }
  for (int i = tid; i < sw.seq_bytes; i += kEncThreads) slot[3 + h2.block_bytes + i] = lits[nl + i];
  uint8_t* d = slot + 3 + h2.prefix_bytes;
  if (h2.type == kRaw) {
    for (int i = tid; i < nl; i += kEncThreads) d[i] = lits[i];
  } else if (h2.type == kCompressed) {
    pack_streams(h2, win, nl, d, [&](int i) { return lits[i]; });
  }
}

// ---- pack: the frames of a call from its slots, for a container C of dsx_blosc_frame.h -------------------------------
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

// One workgroup of 256: frame_bytes(sizes of the chunk's slots, chunk bytes, store) per chunk and the exclusive scan
// of these -> offsets.
template <class FrameBytes>
__device__ __forceinline__ void scan_frame_bytes(const PackArgs& a, FrameBytes frame_bytes) {
  __shared__ int64_t part[256];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; a.offsets[0] = 0; }
  __syncthreads();
  const int per = a.nblocks * kSlotsPerBlock;
  for (int c0 = 0; c0 < a.n_chunks; c0 += 256) {
    const int c = c0 + tid;
    int64_t v = c < a.n_chunks ? (int64_t)frame_bytes(a.sizes + (uint64_t)c * per, a.chunk_bytes, a.store) : 0;
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

template <class C>
__global__ void __launch_bounds__(256) k_pack_scan(PackArgs a) {
  scan_frame_bytes(a, [](const uint32_t* ss, uint64_t n, bool store) { return chunk_frame_bytes<C>(ss, n, store); });
}

// grid = chunks x Blosc blocks: the header (block 0), then the block's share of a memcpyed frame, or its block table
// entry and per stream the length and the bytes -- the shuffled source for a stored stream, else C's prefix and the
// stream's slots, word-wise.
template <class C>
__global__ void __launch_bounds__(256) k_pack_copy(PackArgs a) {
  const int tid = threadIdx.x;
  const uint64_t chunk = blockIdx.x / (uint32_t)a.nblocks;
  const int b = (int)(blockIdx.x % (uint32_t)a.nblocks);
  const uint64_t n = a.chunk_bytes;
  const Geometry g(n);
  uint8_t* out = a.frames + a.offsets[chunk];
  const uint64_t fbytes = (uint64_t)(a.offsets[chunk + 1] - a.offsets[chunk]);
  const bool memcpyed = fbytes >= kBloscHeader + n;
  if (b == 0 && tid == 0) blosc_header(out, C::kFlags, 2, n, g.blocksize, fbytes, memcpyed);
  const uint32_t bsize = a.store ? (uint32_t)n : g.bsize(n, b);
  if (memcpyed) {
    const uint8_t* raw = (const uint8_t*)(a.src + chunk * (n / 2));
    const uint64_t o = (uint64_t)b * g.blocksize;
    if (a.store && b > 0) return;
    for (uint32_t i = tid; i < bsize; i += 256) out[kBloscHeader + o + i] = raw[o + i];
    return;
  }
  const uint32_t* ss_chunk = a.sizes + chunk * (uint64_t)(a.nblocks * kSlotsPerBlock);
  uint64_t pos = kBloscHeader + 4ull * g.nblocks;
  for (int k = 0; k < b; ++k) pos += block_bytes<C>(g, n, k, ss_chunk + k * kSlotsPerBlock);
  if (tid == 0) put_le(out + kBloscHeader + 4 * b, pos, 4);
  const uint32_t* ss = ss_chunk + b * kSlotsPerBlock;
  const uint16_t* e = a.src + chunk * (n / 2) + (uint64_t)b * (g.blocksize / 2);
  const int ns = C::streams(g, n, b);
  const uint32_t sn = bsize / (uint32_t)ns;
  for (int j = 0; j < ns; ++j) {
    uint32_t len[C::kParts];  // (read before the stores below: behind a byte store the sizes would be loaded again)
#pragma unroll
    for (int k = 0; k < C::kParts; ++k) len[k] = ss[j + k];
    const uint32_t m = C::stream_bytes(ss, sn, j);
    if (tid == 0) put_le(out + pos, m, 4);
    uint8_t* d = out + pos + 4;
    pos += 4 + m;
    if (m == sn) {  // stored stream: shuffled_byte at s0 ... s0 + sn -- low bytes up to ne, high bytes from there on
      const uint32_t s0 = (uint32_t)j * sn, ne = bsize / 2;
      const uint32_t nlow = s0 >= ne ? 0u : (ne - s0 < sn ? ne - s0 : sn);
      for (uint32_t p = tid; p < nlow; p += 256) d[p] = (uint8_t)(e[s0 + p] & 255u);
      for (uint32_t p = nlow + tid; p < sn; p += 256) d[p] = (uint8_t)(e[s0 + p - ne] >> 8);
      continue;
    }
    if (tid == 0) C::prefix(sn, d);
    d += C::prefix_bytes(sn);
#pragma unroll
    for (int k = 0; k < C::kParts; ++k) {
      const uint32_t* sl = (const uint32_t*)(a.slots + ((uint64_t)blockIdx.x * kSlotsPerBlock + j + k) * kSlotStride);
      for (uint32_t q = tid; 4 * q < len[k]; q += 256) {
        const uint32_t v = sl[q];
        const uint32_t i = 4 * q;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (i + t < len[k]) d[i + t] = (uint8_t)(v >> (8 * t));
      }
      d += len[k];
    }
  }
}

}  // namespace zenc
}  // namespace dsx

#endif  // DSX_ZENC_KERNELS_H
