// dsx_inflate.h -- zlib streams (DEFLATE, RFC 1950 / 1951; also the chunks of a plain-zlib Zarr store) and blosclz
// streams for the Blosc block decoder (task kinds kTaskZlib and kTaskBlosclz of dsx_zdec_task.h).  Shared by the host
// reference (dsx_blosc_decode_ref) and the device kernel (dsx_zdec_kernels.h), like dsx_lz4_dec.h: plain C++ with no
// STL, no allocation and no library call; g++ builds it for the CPU tests (tests/host/zdec_task_check.cpp, also under
// ASan / UBSan).
//
// Both decoders are generators over a byte reader (Lz4Direct on the host, the LDS window of the kernel): inf_step
// yields the next literal, match, stored run or the end of a zlib stream, blosclz_next the next literal run or match
// of a blosclz stream.  Either validates what it yields against the input and the output before a byte of it is
// copied; a malformed stream ends in a status of dsx_zstd_dec.h, never in an access outside either buffer.
//
// On the device every lane of the wave runs the generator on the same values (uniform control flow: the window
// refills and the barriers below are met by all lanes); `w` is true in the one lane that stores into the tables.
#ifndef DSX_INFLATE_H
#define DSX_INFLATE_H

#include "dsx_lz4_dec.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DSX_WAVE_SYNC() __syncthreads()  // the table stores of lane 0 before the loads of the wave
#else
#define DSX_WAVE_SYNC() ((void)0)
#endif
// the generators keep their state (bit reader, window) in registers on the device: no call may take its address
#if defined(__HIP__) || defined(__CUDACC__)
#define DSX_ZHD_FLAT __host__ __device__ __forceinline__
#else
#define DSX_ZHD_FLAT inline
#endif

namespace dsx {
namespace zdec {

// ---- DEFLATE ---------------------------------------------------------------------------------------------------------
constexpr int kInfFastBits = 10;  // codes up to this length decode by one lookup, longer ones canonically
constexpr int kInfMaxBits = 15;
constexpr int kInfMaxLL = 288, kInfMaxDD = 32;  // symbols of the fixed code sets (286 / 287 and 30 / 31 are never valid)

// One code set: fast[low kInfFastBits bits of the stream] = symbol << 4 | code length (0: a longer code, or none),
// and the canonical form: count[len] codes of each length, their symbols in sym[] by (length, symbol).
struct InfCode {
  uint16_t fast[1 << kInfFastBits];
  uint16_t count[kInfMaxBits + 1];
  uint16_t sym[kInfMaxLL];
};
struct InfTables {
  InfCode ll, dd;  // literal / length and distance codes (dd: the code-length code while a dynamic header is read)
  uint16_t offs[kInfMaxBits + 1];
  uint8_t lens[kInfMaxLL + kInfMaxDD];
};

enum InfSet { kInfSetLens = 0, kInfSetLitLen = 1, kInfSetDist = 2 };

DSX_ZHD_FLAT uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) {
    r = (r << 1) | (v & 1u);
    v >>= 1;
  }
  return r;
}

// Code lengths lens[0 .. n) -> h (offs: 16 words of scratch).  zlib's rules (inftrees.c): an over-subscribed set is an
// error; an incomplete one too, except a distance set that is one code of length 1; a distance set may be empty (a
// block of literals only).
DSX_ZHD_FLAT int inf_build(InfCode& h, uint16_t* offs, const uint8_t* lens, int n, int set, bool w) {
  DSX_WAVE_SYNC();  // lens[] is complete; the loads of the tables so far are done
  for (int len = 0; len <= kInfMaxBits; ++len)
    if (w) h.count[len] = 0;
  for (int s = 0; s < n; ++s) {
    const uint32_t len = lens[s];
    const uint16_t c = h.count[len];
    if (w) h.count[len] = (uint16_t)(c + 1);
  }
  for (int i = 0; i < (1 << kInfFastBits); ++i)
    if (w) h.fast[i] = 0;
  DSX_WAVE_SYNC();
  if (h.count[0] == n) return set == kInfSetDist ? kOk : kErrCodes;
  int left = 1, max = 0;
  uint32_t at = 0;
  for (int len = 1; len <= kInfMaxBits; ++len) {
    const int c = h.count[len];
    left = (left << 1) - c;
    if (left < 0) return kErrCodes;
    if (c) max = len;
    if (w) offs[len] = (uint16_t)at;
    at += (uint32_t)c;
  }
  if (left > 0 && !(set == kInfSetDist && max == 1)) return kErrCodes;
  DSX_WAVE_SYNC();
  for (int s = 0; s < n; ++s) {
    const uint32_t len = lens[s];
    if (len == 0) continue;
    const uint16_t v = offs[len];
    if (w) {
      h.sym[v] = (uint16_t)s;
      offs[len] = (uint16_t)(v + 1);
    }
  }
  DSX_WAVE_SYNC();
  uint32_t code = 0, j = 0;
  for (int len = 1; len <= kInfFastBits; ++len) {
    const uint32_t c = h.count[len];
    for (uint32_t k = 0; k < c; ++k, ++j, ++code) {
      const uint16_t e = (uint16_t)((h.sym[j] << 4) | (uint32_t)len);
      for (uint32_t x = bit_reverse(code, len); x < (1u << kInfFastBits); x += 1u << len)
        if (w) h.fast[x] = e;
    }
    code <<= 1;
  }
  DSX_WAVE_SYNC();
  return kOk;
}

// LSB-first bit reader over s[0 .. n) through the byte reader r.  Bits past the end do not exist: get() fails.
template <typename R>
struct InfBits {
  R& r;
  uint32_t n, ip;  // ip: the next byte to load
  uint64_t acc;    // the next nb bits of the stream, bit 0 first
  int nb;
  DSX_ZHD_FLAT void fill() {
    while (nb <= 56 && ip < n) {
      acc |= (uint64_t)r.at(ip++) << nb;
      nb += 8;
    }
  }
  DSX_ZHD_FLAT bool get(int k, uint32_t* v) {  // k <= 16
    if (nb < k) {
      fill();
      if (nb < k) return false;
    }
    *v = (uint32_t)acc & ((1u << k) - 1u);
    acc >>= k;
    nb -= k;
    return true;
  }
  DSX_ZHD_FLAT void drop(int k) {
    acc >>= k;
    nb -= k;
  }
  DSX_ZHD_FLAT uint32_t byte_pos() const { return ip - (uint32_t)nb / 8; }  // of the first byte no bit was taken from
};

// The next symbol of code set h, or minus a status.  Huffman codes are packed starting from their most significant
// bit, so the stream's next bits are the code reversed.
template <typename R>
DSX_ZHD_FLAT int inf_symbol(InfBits<R>& b, const InfCode& h) {
  if (b.nb < kInfMaxBits) b.fill();
  const uint32_t v = (uint32_t)b.acc;  // (bits above nb are 0)
  const uint32_t e = h.fast[v & ((1u << kInfFastBits) - 1u)];
  if (e) {
    const int len = (int)(e & 15u);
    if (len > b.nb) return -kErrTruncated;
    b.drop(len);
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= kInfMaxBits; ++len) {
    code |= (int)((v >> (len - 1)) & 1u);
    const int c = h.count[len];
    if (code - c < first) {
      if (len > b.nb) return -kErrTruncated;
      b.drop(len);
      return h.sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return b.nb < kInfMaxBits ? -kErrTruncated : -kErrCodes;
}

enum InfEvType { kInfLit = 0, kInfMatch = 1, kInfStored = 2, kInfEnd = 3 };
struct InfEv {
  uint32_t type;
  uint32_t a, b;  // kInfLit: the byte; kInfMatch: length, distance; kInfStored: position in the stream, length;
};                // kInfEnd: the Adler-32 the stream states
struct InfState {
  uint32_t op;  // output made once the events so far are executed
  int mode;     // 0: a block header is next, 1: inside a coded block, 2: the trailer is next
  bool last;
};

// position i of a dynamic header's code-length lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (5 bits each)
DSX_ZHD_FLAT uint32_t inf_order(int i) {
  const uint64_t lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) |
                      (6ull << 35) | (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
  const uint64_t hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// zlib header (RFC 1950): deflate, a window of at most 32 KiB, FCHECK, no preset dictionary
template <typename R>
DSX_ZHD_FLAT int inf_start(InfBits<R>& b) {
  uint32_t cmf, flg;
  if (!b.get(8, &cmf) || !b.get(8, &flg)) return kErrTruncated;
  if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0 || (flg & 0x20u)) return kErrHeader;
  return kOk;
}

// The code sets of a block of type 1 (fixed) or 2 (dynamic: read from the stream) into t.  Returns a status.
template <typename R>
DSX_ZHD_FLAT int inf_block_tables(InfBits<R>& b, InfTables& t, uint32_t type, bool w) {
  uint32_t nlen = kInfMaxLL, ndist = kInfMaxDD;
  DSX_WAVE_SYNC();  // the loads of lens[] so far
  if (type == 1) {
    for (uint32_t i = 0; i < nlen; ++i)
      if (w) t.lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
    for (uint32_t i = 0; i < ndist; ++i)
      if (w) t.lens[nlen + i] = 5;
  } else {
    uint32_t ncode;
    if (!b.get(5, &nlen) || !b.get(5, &ndist) || !b.get(4, &ncode)) return kErrTruncated;
    nlen += 257;
    ndist += 1;
    ncode += 4;
    if (nlen > 286 || ndist > 30) return kErrCodes;
    for (int i = 0; i < 19; ++i)
      if (w) t.lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
      uint32_t v;
      if (!b.get(3, &v)) return kErrTruncated;
      if (w) t.lens[inf_order((int)i)] = (uint8_t)v;
    }
    int st = inf_build(t.dd, t.offs, t.lens, 19, kInfSetLens, w);
    if (st) return st;
    // the lengths of both alphabets are one sequence: a repeat may run from the first into the second
    uint32_t prev = 0, eob = 0;
    for (uint32_t i = 0; i < nlen + ndist;) {
      const int s = inf_symbol(b, t.dd);
      if (s < 0) return -s;
      uint32_t rep = 1, val = (uint32_t)s, x = 0;
      if (s == 16) {
        if (i == 0) return kErrCodes;  // nothing to repeat
        if (!b.get(2, &x)) return kErrTruncated;
        rep = 3 + x;
        val = prev;
      } else if (s == 17) {
        if (!b.get(3, &x)) return kErrTruncated;
        rep = 3 + x;
        val = 0;
      } else if (s == 18) {
        if (!b.get(7, &x)) return kErrTruncated;
        rep = 11 + x;
        val = 0;
      }
      if (rep > nlen + ndist - i) return kErrCodes;
      for (uint32_t k = 0; k < rep; ++k, ++i) {
        if (w) t.lens[i] = (uint8_t)val;
        if (i == 256) eob = val;
      }
      prev = val;
    }
    if (eob == 0) return kErrCodes;  // no end-of-block code
  }
  int st = inf_build(t.ll, t.offs, t.lens, (int)nlen, kInfSetLitLen, w);
  if (!st) st = inf_build(t.dd, t.offs, t.lens + nlen, (int)ndist, kInfSetDist, w);
  return st;
}

// The next event of the stream; st.op is moved past it as if it had been executed.  out_n: the bytes the stream must
// produce.  Returns a status.
template <typename R>
DSX_ZHD_FLAT int inf_step(InfBits<R>& b, InfTables& t, InfState& st, uint32_t out_n, InfEv& ev, bool w) {
  for (;;) {
    if (st.mode == 0) {
      uint32_t last, type;
      if (!b.get(1, &last) || !b.get(2, &type)) return kErrTruncated;
      st.last = last != 0;
      if (type == 3) return kErrReserved;
      if (type == 0) {
        uint32_t len, nlen;
        b.drop(b.nb & 7);  // to the next byte
        if (!b.get(16, &len) || !b.get(16, &nlen)) return kErrTruncated;
        if ((len ^ 0xFFFFu) != nlen) return kErrStored;
        const uint32_t pos = b.byte_pos();
        if (len > b.n - pos) return kErrTruncated;
        if (len > out_n - st.op) return kErrOutput;
        ev.type = kInfStored;
        ev.a = pos;
        ev.b = len;
        b.ip = pos + len;
        b.acc = 0;
        b.nb = 0;
        st.op += len;
        st.mode = st.last ? 2 : 0;
        return kOk;
      }
      const int e = inf_block_tables(b, t, type, w);
      if (e) return e;
      st.mode = 1;
    }
    if (st.mode == 1) {
      const int s = inf_symbol(b, t.ll);
      if (s < 0) return -s;
      if (s < 256) {
        if (st.op >= out_n) return kErrOutput;
        ev.type = kInfLit;
        ev.a = (uint32_t)s;
        ev.b = 0;
        st.op += 1;
        return kOk;
      }
      if (s == 256) {
        st.mode = st.last ? 2 : 0;
        continue;
      }
      if (s > 285) return kErrCodes;
      const uint32_t i = (uint32_t)s - 257;  // 0 .. 28
      uint32_t len, x = 0;
      if (i < 8) {
        len = 3 + i;
      } else if (i == 28) {
        len = 258;  // (no extra bits)
      } else {
        const int eb = (int)(i >> 2) - 1;
        if (!b.get(eb, &x)) return kErrTruncated;
        len = 3 + ((4 + (i & 3u)) << eb) + x;
      }
      const int ds = inf_symbol(b, t.dd);
      if (ds < 0) return -ds;
      if (ds > 29) return kErrCodes;
      uint32_t dist = 1 + (uint32_t)ds;
      if (ds >= 4) {
        const int eb = (ds >> 1) - 1;
        if (!b.get(eb, &x)) return kErrTruncated;
        dist = 1 + ((2 + ((uint32_t)ds & 1u)) << eb) + x;
      }
      if (dist > st.op) return kErrOffset;  // (no preset dictionary)
      if (len > out_n - st.op) return kErrOutput;
      ev.type = kInfMatch;
      ev.a = len;
      ev.b = dist;
      st.op += len;
      return kOk;
    }
    // the trailer: the Adler-32 of the output, big-endian, on the next byte; the stream ends with it
    b.drop(b.nb & 7);
    const uint32_t pos = b.byte_pos();
    if (b.n - pos != 4) return kErrTruncated;  // (cut short, or bytes behind the stream: as for a zstd frame)
    ev.type = kInfEnd;
    ev.a = ((uint32_t)b.r.at(pos) << 24) | ((uint32_t)b.r.at(pos + 1) << 16) | ((uint32_t)b.r.at(pos + 2) << 8) |
           (uint32_t)b.r.at(pos + 3);
    ev.b = 0;
    return st.op == out_n ? kOk : kErrOutput;
  }
}

constexpr uint32_t kAdlerMod = 65521;

inline uint32_t adler32_host(const uint8_t* p, uint32_t n) {
  uint32_t a = 1, b = 0;
  for (uint32_t i = 0; i < n;) {
    const uint32_t end = n - i < 5552 ? n : i + 5552;  // (5552 bytes keep b below 2^32)
    for (; i < end; ++i) {
      a += p[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
  }
  return (b << 16) | a;
}

// ---- host build: one whole zlib stream -------------------------------------------------------------------------------
// Stream s[0 .. n) -> out[0 .. out_n), exactly, with its checksum.
inline int inflate_decode(InfTables& t, const uint8_t* s, uint32_t n, uint8_t* out, uint32_t out_n) {
  Lz4Direct r{s};
  InfBits<Lz4Direct> b{r, n, 0, 0, 0};
  InfState st{0, 0, false};
  int e = inf_start(b);
  if (e) return e;
  for (;;) {
    InfEv ev;
    const uint32_t at = st.op;
    e = inf_step(b, t, st, out_n, ev, true);
    if (e) return e;
    if (ev.type == kInfLit) {
      out[at] = (uint8_t)ev.a;
    } else if (ev.type == kInfMatch) {
      run_seq_host(out + at, s, 0, ev.a, ev.b);
    } else if (ev.type == kInfStored) {
      copy_bytes(out + at, s + ev.a, ev.b);
    } else {
      return adler32_host(out, out_n) == ev.a ? kOk : kErrChecksum;
    }
  }
}

// ---- blosclz -----------------------------------------------------------------------------------------------------------
// blosclz (blosclz.c of c-blosc 1.21; dsx_io.h blosclz_decompress is the pinned host route, and this restates it with
// the same checks): instructions led by a control byte c, the first one masked with 31.  c < 32: c + 1 literals
// follow.  c >= 32: a match of length (c >> 5) + 2 -- when the 3-bit field is 7, length bytes follow and add up until
// one is not 255 -- at distance ((c & 31) << 8) + the next byte + 1; the pair (31, 255) announces a far distance: two
// more bytes (big-endian) + 8191 + 1.  Before it reads the bytes of a match the decoder wants two bytes left in the
// stream.  A stream ends after any instruction.
//
// The instruction at ip of a stream of n bytes whose output so far is op of out_n bytes, as an Lz4Seq that is either
// a literal run (ml == 0) or a match (ll == 0): validated, then ip and op are moved past it.  Returns a status.
template <typename R>
DSX_ZHD_FLAT int blosclz_next(R& r, uint32_t n, uint32_t out_n, uint32_t& ip, uint32_t& op, Lz4Seq& q) {
  if (ip >= n) return kErrTruncated;
  uint32_t ctrl = r.at(ip);
  if (ip == 0) ctrl &= 31u;
  ++ip;
  if (ctrl < 32) {
    const uint32_t run = ctrl + 1;
    if (run > n - ip) return kErrTruncated;
    if (run > out_n - op) return kErrOutput;
    q.lit = ip;
    q.ll = run;
    q.ml = 0;
    q.off = 0;
    ip += run;
    op += run;
    return kOk;
  }
  uint32_t len = (ctrl >> 5) - 1, code;
  const uint32_t ofs = (ctrl & 31u) << 8;
  if (len == 6) {
    do {
      if (n - ip < 2) return kErrTruncated;
      code = r.at(ip++);
      len += code;
      if (len > out_n) return kErrOutput;
    } while (code == 255);
  } else if (n - ip < 2) {
    return kErrTruncated;
  }
  code = r.at(ip++);
  len += 3;
  uint32_t dist = ofs + code;
  if (code == 255 && ofs == (31u << 8)) {
    if (n - ip < 2) return kErrTruncated;
    dist = ((uint32_t)r.at(ip) << 8) + (uint32_t)r.at(ip + 1) + 8191;
    ip += 2;
  }
  dist += 1;
  if (len > out_n - op) return kErrOutput;
  if (dist > op) return kErrOffset;
  q.lit = ip;
  q.ll = 0;
  q.ml = len;
  q.off = dist;
  op += len;
  return kOk;
}

// host build: stream s[0 .. n) -> out[0 .. out_n), exactly (a stream of no bytes holds none)
inline int blosclz_decode(const uint8_t* s, uint32_t n, uint8_t* out, uint32_t out_n) {
  Lz4Direct r{s};
  uint32_t ip = 0, op = 0;
  while (ip < n) {
    Lz4Seq q;
    const uint32_t at = op;
    const int st = blosclz_next(r, n, out_n, ip, op, q);
    if (st) return st;
    run_seq_host(out + at, s + q.lit, q.ll, q.ml, q.off);  // (a literal run or a match)
  }
  return op == out_n ? kOk : kErrOutput;
}

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_INFLATE_H
