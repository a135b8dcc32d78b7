// dsx_zdec_kernels.h -- Blosc blocks decoded on the device (dsx_blosc_decode_device): one wave per task of
// dsx_io_read_frames (dsx_zdec_task.h: DecTask, the kinds and flags; run_task_host is the same flow on the host).
//
//   k_zdec, k_zdec_all   grid = tasks, 64 threads each.  Both are zdec_task: k_zdec_all runs the zlib and blosclz
//            tasks, k_zdec every other kind, and the wave of the other kernel leaves at once (all four decoders in one
//            kernel need 255 VGPRs and scratch).  One int32 status per task (dsx_zstd_dec.h Status; 0 = exact output).
//
//   zdec_task    fill, or copy / stored bytes (wide copies), or the streams of the block one after the other -- a
//            split block has two, each stored or coded -- into the output, or into scratch when an un-shuffle follows
//            (2-byte: wave_unshuffle; bit: wave_unbitshuffle, 8 x 8 bit transposes, 8 elements per lane and round).
//
//   The four stream drivers parse with the primitives of the codec headers and execute with:
//     wave_copy / wave_pattern   a copy by the whole wave, 8 loads in flight per lane; a match that overlaps itself.
//     wave_match     one match behind the watermark: the wave keeps the offset `fenced` below which its output was
//                    made visible by the last barrier (whose workgroup-scope fence orders the global stores before
//                    the loads that follow) and passes another barrier only when the match source reaches above it
//                    (match_needs_fence of dsx_zdec_task.h, which the walker of tests/host/zstd_dec_check.cpp replays).
//     Lz4Window      the stream bytes of a parser that every lane runs alike: a window of kLz4Win bytes in LDS (the
//                    reads are broadcasts) that the wave refills together when the parse leaves it.
//   zstd_wave    lane 0 parses the headers and builds the Huffman and FSE tables in LDS; the four literal streams
//            are decoded by lanes 0 .. 3 into the end of the stream's output, reading their bits from LDS, where the
//            wave stages kLitWin bytes of each stream per round; lane 0 decodes and validates a batch of up to kSeqBatch
//            sequences into LDS and the wave runs it, the literals from the end of the output (or from the frame: raw).
//   lz_wave      LZ4 (lz4_next) and blosclz (blosclz_next) have no tables: every lane parses the same sequence
//            through an Lz4Window, then the wave copies the literals -- out of the window when they lie in it -- and
//            the match.
//   inflate_wave zlib: literals and matches are interleaved in one bit stream, so every lane runs the same parse
//            (inf_step) through an Lz4Window -- lane 0 alone stores the code tables, which share the LDS of the zstd
//            tables -- into a batch of sequences and a literal window in LDS, then the wave runs the batch; a stored
//            block is one wide copy.  The Adler-32 of the stream is checked against the bytes the wave made.
#ifndef DSX_ZDEC_KERNELS_H
#define DSX_ZDEC_KERNELS_H

#include <hip/hip_runtime.h>

#include "dsx_zdec_task.h"

namespace dsx {
namespace zdec {

constexpr int kDecThreads = 64;  // one wave per task
constexpr int kSeqBatch = 128;
constexpr int kLitWin = 2048;    // bytes of each literal stream staged in LDS per round

struct DecArgs {
  const uint8_t* packed;
  const DecTask* tasks;
  uint8_t* out;      // the bricks
  uint8_t* scratch;  // shuffled tasks decode here first (same offsets as out)
  int32_t* status;
  uint64_t packed_bytes, out_bytes;
};

// n bytes src -> dst by the wave, 8 loads in flight per lane.  Rounds go forward in step for the whole wave and every
// load of a round precedes its stores, so dst may overlap src from below (dst <= src: the literal copies out of the
// end of the output).
__device__ inline void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n, int lane) {
  uint32_t base = 0;
  for (; base + 8 * 64 <= n; base += 8 * 64) {
    uint8_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[base + (uint32_t)lane + 64u * u];
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[base + (uint32_t)lane + 64u * u] = v[u];
  }
  for (; base < n; base += 64)
    if (base + (uint32_t)lane < n) dst[base + (uint32_t)lane] = src[base + (uint32_t)lane];
}

// match of ml bytes at dst whose source starts `off` bytes back, off < ml: the last `off` bytes repeat
__device__ inline void wave_pattern(uint8_t* dst, uint32_t off, uint32_t ml, int lane) {
  const uint8_t* src = dst - off;
  uint32_t jj = (uint32_t)lane % off;
  const uint32_t step = 64u % off;
  uint32_t i = (uint32_t)lane;
  for (; i + 3 * 64 < ml; i += 4 * 64) {
    uint8_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = src[jj];
      jj += step;
      if (jj >= off) jj -= off;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[i + 64 * u] = v[u];
  }
  for (; i < ml; i += 64) {
    dst[i] = src[jj];
    jj += step;
    if (jj >= off) jj -= off;
  }
}

// The match of ml bytes at o + wop whose source starts `off` bytes back, behind the watermark `fenced` (uniform: every
// lane runs the same sequence)
__device__ __forceinline__ void wave_match(uint8_t* o, uint32_t wop, uint32_t off, uint32_t ml, uint32_t& fenced, int lane) {
  const uint32_t src = wop - off;
  if (match_needs_fence(src, ml, off, fenced)) {
    __syncthreads();  // earlier stores before the match loads
    fenced = wop;
  }
  if (off >= ml) wave_copy(o + wop, o + src, ml, lane);
  else wave_pattern(o + wop, off, ml, lane);  // overlapping: the last `off` bytes repeat
}

// 2-byte un-shuffle of n bytes s -> d (bytes [0, n/2) are the low bytes; an odd tail byte as is)
__device__ inline void wave_unshuffle(uint8_t* d, const uint8_t* s, uint32_t n, int lane) {
  const uint32_t ne = n / 2;
  if ((((uintptr_t)d | (uintptr_t)s | ne) & 3u) == 0) {
    const uint32_t* lo = (const uint32_t*)s;
    const uint32_t* hi = (const uint32_t*)(s + ne);
    uint2* d8 = (uint2*)d;
    for (uint32_t q = (uint32_t)lane; q < ne / 4; q += 64) {
      const uint32_t a = lo[q], b = hi[q];
      const uint32_t w0 = (a & 0xFFu) | ((b & 0xFFu) << 8) | ((a & 0xFF00u) << 8) | ((b & 0xFF00u) << 16);
      const uint32_t w1 = ((a >> 16) & 0xFFu) | (((b >> 16) & 0xFFu) << 8) | ((a >> 24) << 16) | ((b >> 24) << 24);
      d8[q] = make_uint2(w0, w1);
    }
  } else {
    for (uint32_t i = (uint32_t)lane; i < ne; i += 64) {
      d[2 * i] = s[i];
      d[2 * i + 1] = s[ne + i];
    }
  }
  if ((n & 1u) && lane == 0) d[n - 1] = s[n - 1];
}

// bit un-shuffle of n bytes s -> d (dsx_zdec_task.h unbitshuffle8: 8 elements = 16 bytes per lane and round)
__device__ __forceinline__ void wave_unbitshuffle(uint8_t* d, const uint8_t* s, uint32_t n, int lane) {
  if (!bitshuffled(n)) {
    wave_copy(d, s, n, lane);
    return;
  }
  const uint32_t row = n / 16;
  const bool wide = ((uintptr_t)d & 15u) == 0;
  for (uint32_t j = (uint32_t)lane; j < row; j += 64) {
    uint64_t w0, w1;
    unbitshuffle8(s, row, j, &w0, &w1);
    if (wide) {
      ((uint4*)d)[j] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    } else {
      for (int i = 0; i < 8; ++i) {
        d[16 * j + (uint32_t)i] = (uint8_t)(w0 >> (8 * i));
        d[16 * j + 8 + (uint32_t)i] = (uint8_t)(w1 >> (8 * i));
      }
    }
  }
  if ((n & 1u) && lane == 0) d[n - 1] = s[n - 1];
}

// LDS of one wave: the tables and staging of the zstd decoder; an LZ4 or blosclz stream stages its window in lbuf; a
// zlib stream has its tables in the place of the zstd tables, its window in lbuf[0] and its literals in lbuf[2 .. 3]
struct WaveLds {
  union {
    Tables t;
    InfTables inf;
  };
  Seq batch[kSeqBatch];
  Streams ss;
  int32_t sh_st, sh_cnt, sh_lst[4];
  uint32_t sh_u[8];  // broadcast scalars of lane 0
  uint32_t sh_blo[4];
  uint8_t lbuf[4][kLitWin];
};

constexpr uint32_t kLz4Win = 2048;  // bytes of an LZ4 stream staged in LDS (within WaveLds::lbuf)
constexpr uint32_t kInfLitWin = 4096;  // literals of a batch of a zlib stream (WaveLds::lbuf[2 .. 3])
static_assert(kLz4Win <= kLitWin && kInfLitWin <= 2 * kLitWin, "the windows lie in WaveLds::lbuf");
static_assert(kLz4Win % 512 == 0 && kLitWin % 512 == 0, "the staging loops store whole rounds of 512 bytes");
static_assert(sizeof(WaveLds::batch) >= 2 * 64 * sizeof(uint32_t), "wave_adler32 reduces in WaveLds::batch");

// The bytes of a stream for a parser that every lane runs alike (lz4_next, blosclz_next, inf_step): a window
// [lo, lo + cnt) of the stream in LDS that the wave refills together (uniform control flow) at the first byte asked
// for outside it.
struct Lz4Window {
  const uint8_t* s;
  uint32_t n;
  uint8_t* win;
  uint32_t lo, cnt;
  int lane;
  __device__ __forceinline__ uint8_t at(uint32_t p) {  // p < n
    if (p - lo >= cnt) {
      __syncthreads();  // the reads of the window so far
      lo = p;
      cnt = n - p < kLz4Win ? n - p : kLz4Win;
      for (uint32_t i0 = 0; i0 < cnt; i0 += 8 * 64) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint32_t i = i0 + (uint32_t)lane + 64u * u;
          v[u] = i < cnt ? s[p + i] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) win[i0 + (uint32_t)lane + 64u * u] = v[u];  // (kLz4Win is a multiple of 512)
      }
      __syncthreads();
    }
    return win[p - lo];
  }
};

// One bare LZ4 block (lz4_next: sequences of literals and a match, the last one without a match) or one blosclz stream
// (kBlosclz, blosclz_next: instructions that are a literal run or a match, until the bytes end) s[0 .. n) ->
// o[0 .. out_n) by the wave; returns a status (the same in every lane)
template <bool kBlosclz>
__device__ __forceinline__ int lz_wave(uint8_t* win, const uint8_t* s, uint32_t n, uint8_t* o, uint32_t out_n, int lane) {
  Lz4Window r{s, n, win, 0, 0, lane};
  uint32_t ip = 0, op = 0, fenced = 0;
  while (!kBlosclz || ip < n) {
    Lz4Seq q;
    const uint32_t at = op;
    int st;
    if constexpr (kBlosclz) st = blosclz_next(r, n, out_n, ip, op, q);
    else st = lz4_next(r, n, out_n, ip, op, q);
    if (st) return st;
    if (!kBlosclz || q.ml == 0) {  // (a blosclz instruction is a literal run or a match)
      if (q.lit >= r.lo && q.lit - r.lo + q.ll <= r.cnt) {  // the literals are staged: stores only
        const uint8_t* w = win + (q.lit - r.lo);
        for (uint32_t i = (uint32_t)lane; i < q.ll; i += 64) o[at + i] = w[i];
      } else {
        wave_copy(o + at, s + q.lit, q.ll, lane);
      }
    }
    if (q.ml == 0) {
      if constexpr (kBlosclz) continue;
      else break;  // the last sequence of an LZ4 block
    }
    wave_match(o, kBlosclz ? at : at + q.ll, q.off, q.ml, fenced, lane);
  }
  return op == out_n ? kOk : kErrOutput;
}

// Adler-32 of p[0 .. n), bytes the wave stored before the last barrier: lane l sums the bytes l, l + 64, ... with
// their weights n - i (mod 65521, kept by stepping), the wave adds up through red (2 x 64 words of LDS)
__device__ inline uint32_t wave_adler32(uint32_t* red, const uint8_t* p, uint32_t n, int lane) {
  uint64_t a = 0, b = 0;
  uint32_t wgt = (uint32_t)lane < n ? (n - (uint32_t)lane) % kAdlerMod : 0u;
  for (uint32_t i = (uint32_t)lane; i < n; i += 64) {
    const uint32_t v = p[i];
    a += v;
    b += (uint64_t)wgt * v;
    wgt = wgt >= 64 ? wgt - 64 : wgt + kAdlerMod - 64;
  }
  red[lane] = (uint32_t)(a % kAdlerMod);
  red[64 + lane] = (uint32_t)(b % kAdlerMod);
  __syncthreads();
  uint32_t sa = 1, sb = n % kAdlerMod;
  for (int l = 0; l < 64; ++l) {
    sa += red[l];       // (64 terms below 2^16: no overflow)
    sb += red[64 + l];
  }
  __syncthreads();  // red may be written again
  return ((sb % kAdlerMod) << 16) | (sa % kAdlerMod);
}

// One zlib stream s[0 .. n) -> o[0 .. out_n) by the wave; returns a status (the same in every lane)
__device__ __forceinline__ int inflate_wave(WaveLds& sh, const uint8_t* s, uint32_t n, uint8_t* o, uint32_t out_n, int lane) {
  Lz4Window r{s, n, &sh.lbuf[0][0], 0, 0, lane};
  InfBits<Lz4Window> b{r, n, 0, 0, 0};
  InfState st{0, 0, false};
  uint8_t* lw = &sh.lbuf[2][0];
  Seq* batch = sh.batch;
  const bool w = lane == 0;
  int e = inf_start(b);
  if (e) return e;
  uint32_t wop = 0, fenced = 0, adler = 0;
  for (;;) {
    // every lane parses the same events: matches into the batch with the literals before them, until the batch or the
    // literal window is full or an event is none of the two
    uint32_t c = 0, nl = 0, ll = 0;
    InfEv ev;
    ev.type = kInfLit;
    while (c < (uint32_t)kSeqBatch && nl < kInfLitWin) {
      e = inf_step(b, sh.inf, st, out_n, ev, w);
      if (e) return e;  // (uniform)
      if (ev.type == kInfLit) {
        if (w) lw[nl] = (uint8_t)ev.a;
        ++nl;
        ++ll;
      } else if (ev.type == kInfMatch) {
        if (w) batch[c] = Seq{ll, ev.a, ev.b};
        ++c;
        ll = 0;
      } else {
        break;
      }
    }
    __syncthreads();  // the batch and its literals
    uint32_t lp = 0;
    for (uint32_t j = 0; j < c; ++j) {
      const Seq q = batch[j];
      for (uint32_t i = (uint32_t)lane; i < q.ll; i += 64) o[wop + i] = lw[lp + i];
      wop += q.ll;
      lp += q.ll;
      wave_match(o, wop, q.off, q.ml, fenced, lane);
      wop += q.ml;
    }
    for (uint32_t i = (uint32_t)lane; i < ll; i += 64) o[wop + i] = lw[lp + i];  // the literals behind the last match
    wop += ll;
    if (ev.type == kInfStored) {
      wave_copy(o + wop, s + ev.a, ev.b, lane);
      wop += ev.b;
    }
    __syncthreads();  // the batch may be refilled; the stores above are visible
    fenced = wop;
    if (ev.type == kInfEnd) {
      adler = ev.a;
      break;
    }
  }
  return wave_adler32((uint32_t*)sh.batch, o, out_n, lane) == adler ? kOk : kErrChecksum;
}

// One zstd frame s[0 .. n) -> o[0 .. out_n) by the wave; returns a status (the same in every lane)
__device__ __forceinline__ int zstd_wave(WaveLds& sh, const uint8_t* s, uint32_t n, uint8_t* o, uint32_t out_n, int lane) {
  Tables& t = sh.t;
  Seq* batch = sh.batch;
  Streams& ss = sh.ss;
  int32_t &sh_st = sh.sh_st, &sh_cnt = sh.sh_cnt;
  int32_t* sh_lst = sh.sh_lst;
  uint32_t *sh_u = sh.sh_u, *sh_blo = sh.sh_blo;
  uint8_t(*lbuf)[kLitWin] = sh.lbuf;
  SeqState q;  // lane 0's sequence decoder (its repeat offsets live for the frame)
  if (lane == 0) {
    FrameHdr fh;
    int st = frame_header(s, n, fh);
    if (!st && fh.content >= 0 && fh.content != (int64_t)out_n) st = kErrOutput;
    t.huf_log = 0;
    t.ll_log = t.of_log = t.ml_log = -1;
    q.rep0 = 1; q.rep1 = 4; q.rep2 = 8;
    sh_st = st;
    sh_u[0] = st ? 0u : fh.bytes;
  }
  __syncthreads();
  int st = sh_st;
  uint32_t ip = sh_u[0], op = 0;
  while (!st) {
    // ---- block header (lane 0) and the literals section
    if (lane == 0) {
      int e = kOk;
      uint32_t bh = 0;
      if (n - ip < 3) e = kErrTruncated;
      else bh = le(s + ip, 3);
      const uint32_t type = (bh >> 1) & 3, bs = bh >> 3;
      if (!e && type == 3) e = kErrReserved;
      if (!e && bs > kBlockMax) e = kErrBlockSize;
      if (!e && type == 0 && (bs > n - ip - 3)) e = kErrTruncated;
      if (!e && type == 1 && n - ip - 3 < 1) e = kErrTruncated;
      if (!e && type < 2 && bs > out_n - op) e = kErrOutput;
      if (!e && type == 2 && bs > n - ip - 3) e = kErrTruncated;
      sh_u[1] = bh;
      if (!e && type == 2) {  // literals: header, tree, streams
        const uint8_t* b = s + ip + 3;
        LitHdr lh;
        e = lit_header(b, bs, lh);
        if (!e && lh.regen > out_n - op) e = kErrOutput;
        uint32_t tree = 0;
        if (!e && lh.type == 2) {
          const int used = read_huf_tree(t, b + lh.hdr, lh.csize);
          if (used < 0) e = -used;
          else tree = (uint32_t)used;
        } else if (!e && lh.type == 3 && t.huf_log == 0) {
          e = kErrHuffman;
        }
        if (!e && lh.type >= 2) e = split_streams(b + lh.hdr + tree, lh.csize - tree, lh.regen, lh.streams, ss);
        sh_u[2] = (uint32_t)lh.type;
        sh_u[3] = lh.regen;
        sh_u[4] = lh.hdr + tree;                     // the literals (raw) or the streams start here in the block
        sh_u[5] = lh.hdr + lh.csize;                 // the sequences section starts here
        sh_u[6] = lh.type >= 2 ? (uint32_t)lh.streams : 0u;
      }
      sh_st = e;
    }
    __syncthreads();
    st = sh_st;
    if (st) break;
    const uint32_t bh = sh_u[1], type = (bh >> 1) & 3, bs = bh >> 3;
    const bool last = bh & 1;
    ip += 3;
    if (type == 0) {
      wave_copy(o + op, s + ip, bs, lane);
      ip += bs;
      op += bs;
    } else if (type == 1) {
      const uint8_t v = s[ip];
      for (uint32_t i = (uint32_t)lane; i < bs; i += 64) o[op + i] = v;
      ip += 1;
      op += bs;
    } else {
      const uint8_t* b = s + ip;
      const uint32_t lt = sh_u[2], regen = sh_u[3], lit_at = sh_u[4], seq_at = sh_u[5];
      const int streams = (int)sh_u[6];
      uint8_t* lit_dst = o + (out_n - regen);
      const uint8_t* lit = lt == 0 ? b + lit_at : lit_dst;
      if (lt == 1) {
        const uint8_t v = b[lit_at];  // the RLE byte follows the header
        for (uint32_t i = (uint32_t)lane; i < regen; i += 64) lit_dst[i] = v;
      } else if (lt >= 2) {
        // lanes 0 .. streams-1 decode one stream each (dsx_zstd_dec.h huf_stream) from bytes the wave stages in LDS,
        // kLitWin per stream and round, the top of what each lane has not read yet
        const uint8_t* base = b + lit_at + (lane < streams ? ss.off[lane] : 0u);
        const uint32_t len = lane < streams ? ss.len[lane] : 0u;
        uint32_t left = lane < streams ? ss.cnt[lane] : 0u;
        uint8_t* dst = lit_dst;
        for (int j = 0; j < lane && j < streams; ++j) dst += ss.cnt[j];
        int lst = kOk;
        int64_t pos = 0;    // unread bits of the stream: [0, pos)
        uint64_t acc = 0;   // its top `avail` bits, [pos - avail, pos); pos - avail is a byte boundary
        int avail = 0;
        if (lane < streams) {
          if (len == 0 || base[len - 1] == 0) {
            lst = kErrBitstream;
          } else {
            avail = hibit(base[len - 1]);
            pos = 8 * (int64_t)(len - 1) + avail;
            acc = base[len - 1] & ((1u << avail) - 1u);
          }
        }
        const int log = t.huf_log;
        for (;;) {
          const bool act = lane < streams && lst == kOk && left > 0;
          uint32_t blo = 0;
          if (act) {
            const int64_t top = (pos - avail) / 8;  // bytes [0, top) are still to be read
            blo = top > kLitWin ? (uint32_t)(top - kLitWin) : 0u;
          }
          if (lane < 4) {
            sh_lst[lane] = act ? 1 : 0;
            sh_blo[lane] = blo;
          }
          __syncthreads();
          const int any = sh_lst[0] | sh_lst[1] | sh_lst[2] | sh_lst[3];
          if (!any) break;
          for (int j = 0; j < streams; ++j) {
            if (!sh_lst[j]) continue;
            const uint8_t* sb = b + lit_at + ss.off[j];
            const uint32_t lo = sh_blo[j], sl = ss.len[j];
            for (uint32_t i0 = 0; i0 < (uint32_t)kLitWin; i0 += 8 * 64) {
              uint8_t v[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const uint32_t q = lo + i0 + (uint32_t)lane + 64u * u;
                v[u] = q < sl ? sb[q] : (uint8_t)0;
              }
#pragma unroll
              for (int u = 0; u < 8; ++u) lbuf[j][i0 + (uint32_t)lane + 64u * u] = v[u];
            }
          }
          __syncthreads();
          if (act) {
            const uint8_t* buf = lbuf[lane];
            const uint32_t mask = (1u << log) - 1u;
            while (left > 0) {
              if (avail < log) {
                int64_t q = (pos - avail) / 8;
                if (blo > 0 && q < (int64_t)blo + 8) break;  // the next bytes are below the staged ones
                while (avail <= 56 && q > 0) {
                  --q;
                  acc = (acc << 8) | buf[q - blo];
                  avail += 8;
                }
              }
              const uint32_t idx = avail >= log ? (uint32_t)(acc >> (avail - log)) & mask
                                                : (uint32_t)(acc << (log - avail)) & mask;  // zeros below bit 0
              const HufEntry e = t.huf[idx];
              *dst++ = e.sym;
              --left;
              pos -= e.nb;
              if (pos < 0) {
                lst = kErrBitstream;
                break;
              }
              avail -= e.nb;
            }
            if (lst == kOk && left == 0 && pos != 0) lst = kErrBitstream;
          }
          __syncthreads();  // the staged bytes may be replaced
        }
        if (lane < streams) sh_lst[lane] = lst;
      }
      __syncthreads();  // the literals are visible to the wave
      if (lane == 0) {
        int e = kOk;
        for (int j = 0; j < streams && !e; ++j) e = sh_lst[j];
        uint32_t nseq = 0;
        q.op = op;
        q.lit_used = 0;
        q.nlit = regen;
        if (!e) e = seq_header(t, b + seq_at, bs - seq_at, q, &nseq);
        if (!e) q.left = nseq;
        else q.left = 0;
        sh_st = e;
        sh_u[7] = nseq;
      }
      __syncthreads();
      st = sh_st;
      if (st) break;
      const uint32_t nseq = sh_u[7];
      uint32_t wop = op, lp = 0, fenced = op;
      for (uint32_t done = 0; done < nseq;) {
        if (lane == 0) {
          int e = kOk, c = 0;
          while (c < kSeqBatch && done + (uint32_t)c < nseq) {
            Seq e1;
            e = next_seq(t, q, out_n, e1);
            if (e) break;
            batch[c++] = e1;
          }
          if (!e && done + (uint32_t)c == nseq) e = seq_end(q);
          sh_st = e;
          sh_cnt = c;
        }
        __syncthreads();
        const int c = sh_cnt;
        for (int j = 0; j < c; ++j) {
          const Seq e1 = batch[j];
          wave_copy(o + wop, lit + lp, e1.ll, lane);  // (writes stay below the literals not yet read)
          wop += e1.ll;
          lp += e1.ll;
          wave_match(o, wop, e1.off, e1.ml, fenced, lane);
          wop += e1.ml;
        }
        done += (uint32_t)c;
        st = sh_st;
        __syncthreads();  // the batch may be refilled; the stores above are visible
        fenced = wop;
        if (st) break;
      }
      if (st) break;
      // trailing literals
      const uint32_t rest = regen - lp;
      if (rest > out_n - wop || wop + rest - op > kBlockMax) {
        st = rest > out_n - wop ? kErrOutput : kErrBlockSize;
        break;
      }
      wave_copy(o + wop, lit + lp, rest, lane);
      op = wop + rest;
      ip += bs;
    }
    __syncthreads();  // this block's output is visible to the next block's matches
    if (last) break;
  }
  if (!st && op != out_n) st = kErrOutput;
  if (!st && ip != n) st = kErrTruncated;
  return st;
}

// One task by one wave (run_task_host of dsx_zdec_task.h is this flow on the host).  kAll: the kernel of the zlib and
// blosclz tasks (k_zdec_all); the tasks of the other kernel are left alone, their status too.
template <bool kAll>
__device__ __forceinline__ void zdec_task(const DecArgs& a) {
  __shared__ WaveLds sh;
  const int lane = threadIdx.x;
  const DecTask k = a.tasks[blockIdx.x];
  const uint32_t kind = k.kind & kTaskKindMask;
  if ((kind == kTaskZlib || kind == kTaskBlosclz) != kAll) return;
  const bool split = (k.kind & kTaskSplit) != 0, bits = (k.kind & kTaskBitshuffle) != 0;
  const bool shuf = !bits && (k.kind & kTaskShuffle) != 0;
  const uint32_t out_n = k.dst_len, n = k.src_len;
  if (k.dst > a.out_bytes || out_n > a.out_bytes - k.dst ||
      (kind != kTaskFill && (k.src > a.packed_bytes || n > a.packed_bytes - k.src))) {
    if (lane == 0) a.status[blockIdx.x] = kErrOutput;
    return;
  }
  uint8_t* d = a.out + k.dst;
  if (kind == kTaskFill) {
    for (uint32_t i = (uint32_t)lane; i < out_n; i += 64) d[i] = (uint8_t)(k.src >> (8 * (i & 1)));
    if (lane == 0) a.status[blockIdx.x] = kOk;
    return;
  }
  const uint8_t* s = a.packed + k.src;
  const bool plain = !split && (kind == kTaskCopy || kind == kTaskStored);  // the bytes are there: un-shuffle or copy
  if (!kAll && !plain && kind != kTaskZstd && kind != kTaskLz4) {
    if (lane == 0) a.status[blockIdx.x] = kErrReserved;
    return;
  }
  uint8_t* o = (shuf || bits) ? a.scratch + k.dst : d;
  // the streams of the block one after the other, each into its share of the block: a split block holds a low-byte
  // and a high-byte stream behind an int32 length each (a length of the whole share: stored), any other block is
  // its one stream
  const uint32_t nstreams = split ? kSplitStreams : 1u;
  const uint32_t ne = out_n / nstreams;
  int st = out_n % nstreams ? kErrOutput : kOk;
  if (plain && n != out_n) st = kErrOutput;
  uint32_t pos = 0;
  for (uint32_t j = 0; j < nstreams && !st && !plain; ++j) {
    uint32_t at = 0, len = n;
    if (split) {
      st = split_stream(s, n, &pos, &at, &len);
      if (st) break;
      __syncthreads();  // the LDS of the stream before
    }
    if (split && len == ne) wave_copy(o + j * ne, s + at, ne, lane);  // stored
    else if constexpr (kAll) {
      if (kind == kTaskZlib) st = inflate_wave(sh, s + at, len, o + j * ne, ne, lane);
      else st = lz_wave<true>(&sh.lbuf[0][0], s + at, len, o + j * ne, ne, lane);
    } else {
      if (kind == kTaskZstd) st = zstd_wave(sh, s + at, len, o + j * ne, ne, lane);
      else st = lz_wave<false>(&sh.lbuf[0][0], s + at, len, o + j * ne, ne, lane);
    }
  }
  if (split && !st && pos != n) st = kErrTruncated;
  if (!st) {
    const uint8_t* from = plain ? s : o;
    if (shuf || bits) {
      __syncthreads();  // the decoded bytes are visible to the wave
      if (bits) wave_unbitshuffle(d, from, out_n, lane);
      else wave_unshuffle(d, from, out_n, lane);
    } else if (plain) {
      wave_copy(d, s, n, lane);
    }
  }
  if (lane == 0) a.status[blockIdx.x] = st;
}

__global__ void __launch_bounds__(kDecThreads) k_zdec(DecArgs a) { zdec_task<false>(a); }
__global__ void __launch_bounds__(kDecThreads) k_zdec_all(DecArgs a) { zdec_task<true>(a); }

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_ZDEC_KERNELS_H
