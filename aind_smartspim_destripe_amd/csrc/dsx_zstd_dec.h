// dsx_zstd_dec.h -- zstd frame decoder (RFC 8878) shared by the host reference (dsx_blosc_decode_ref) and the device
// kernels (dsx_zdec_kernels.h): the format primitives, which both builds run, and decode_frame, the host decoder of one
// frame.  The statuses of every codec of the Blosc block decoder are here too; the tasks around a frame are
// dsx_zdec_task.h.  Plain C++ with no STL and no allocation; g++ builds it for the CPU tests
// (tests/host/zstd_dec_check.cpp, also under ASan / UBSan).
//
// One frame decodes into a caller-given output of exactly the expected size.  Supported: single-segment and window
// descriptor frame headers with every Frame_Content_Size width; Raw, RLE and Compressed blocks (<= 128 KiB); Raw, RLE,
// Huffman and Treeless literals in 1 or 4 streams, weights direct or FSE-coded, code lengths <= 11 bits; sequences
// with Predefined, RLE, FSE_Compressed and Repeat modes for each of literal lengths, offsets and match lengths, repeat
// offsets, overlapping matches and matches into earlier blocks.  A dictionary ID or a checksum is "unsupported".
//
// Safety: every read is bounded by the input length and every write by the output length; malformed input ends in a
// status code, never in an assert or a trap (the device reads bytes from files on disk).
//
// Layout of the work: the literals of a compressed block are decoded into the END of the frame's output (a valid
// block regenerates at least as many bytes as it has literals, and the sequences write strictly below the literals
// they have not consumed yet), so no separate literal buffer is needed; Raw literals are read in place.  Each sequence
// is decoded and validated (literal count, offset against the output so far, output bound) before any byte of it is
// written: the host build executes it at once, the device kernel queues a batch of them for the whole wave.
#ifndef DSX_ZSTD_DEC_H
#define DSX_ZSTD_DEC_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define DSX_ZHD __host__ __device__
#else
#define DSX_ZHD
#endif

namespace dsx {
namespace zdec {

enum Status {
  kOk = 0,
  kErrTruncated = 1,     // the input ends inside a header, a table or a block
  kErrMagic = 2,         // not a zstd frame
  kErrUnsupported = 3,   // dictionary ID or content checksum
  kErrReserved = 4,      // a reserved bit or field is set (frame descriptor, block type, sequence modes)
  kErrBlockSize = 5,     // block larger than 128 KiB
  kErrLiterals = 6,      // literals section malformed, or more literals than the block may hold
  kErrHuffman = 7,       // Huffman tree description malformed, or weights over the 11-bit limit
  kErrAccuracy = 8,      // FSE accuracy log above the limit of its table
  kErrFse = 9,           // FSE table description malformed
  kErrBitstream = 10,    // a bitstream overruns its bytes or is not consumed exactly
  kErrOffset = 11,       // a match offset reaches before the start of the output
  kErrOutput = 12,       // output longer or shorter than expected
  kErrSequences = 13,    // a sequence takes more literals than the block has, or a bad code
  // dsx_inflate.h (zlib streams)
  kErrChecksum = 14,     // the Adler-32 of the stream is not that of the bytes produced
  kErrCodes = 15,        // a Huffman code set is over-subscribed, incomplete or lacks the end-of-block code; a code
                         // that stands for no symbol; a length symbol above 285 or a distance symbol above 29
  kErrStored = 16,       // LEN and NLEN of a stored block are not complements
  kErrHeader = 17,       // zlib header: method, window, FCHECK, or a preset dictionary
};

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint32_t kBlockMax = 128 * 1024;
constexpr int kHufMaxBits = 11;
constexpr int kMaxLL = 35, kMaxML = 52, kMaxOF = 31;
constexpr int kLogLL = 9, kLogML = 9, kLogOF = 8, kLogWt = 6;

struct HufEntry {
  uint8_t sym, nb;
};
struct FseEntry {
  uint16_t base;  // next state = base + bits(nb)
  uint8_t sym, nb;
};

// Tables and scratch of one frame (LDS on the device, ~10 KB).  Tables persist across the blocks of the frame
// (Treeless literals and Repeat modes).
struct Tables {
  HufEntry huf[1 << kHufMaxBits];
  FseEntry ll[1 << kLogLL], of[1 << kLogOF], ml[1 << kLogML], wt[1 << kLogWt];
  int16_t norm[64];
  uint16_t sdesc[64];
  uint8_t w[256];  // Huffman weights
  uint16_t rank[kHufMaxBits + 2];
  int huf_log;     // 0: no Huffman table yet
  int ll_log, of_log, ml_log;  // -1: no table yet
};

DSX_ZHD inline int hibit(uint32_t v) {  // v > 0
  int r = 0;
  while (v >>= 1) ++r;
  return r;
}
DSX_ZHD inline uint32_t le(const uint8_t* p, int n) {
  uint32_t v = 0;
  for (int i = n - 1; i >= 0; --i) v = (v << 8) | p[i];
  return v;
}

// How every host decoder (decode_frame, lz4_decode, inflate_decode, blosclz_decode) executes what it has validated:
// ll literals to d, then a match of ml bytes whose source starts `off` bytes back, byte by byte (off < ml: the match
// overlaps itself and repeats its last `off` bytes)
inline void copy_bytes(uint8_t* d, const uint8_t* s, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) d[i] = s[i];
}
inline void run_seq_host(uint8_t* d, const uint8_t* lit, uint32_t ll, uint32_t ml, uint32_t off) {
  copy_bytes(d, lit, ll);
  d += ll;
  for (uint32_t i = 0; i < ml; ++i) d[i] = d[(int64_t)i - (int64_t)off];
}

// Backward bit reader over s[0 .. n): bits [0, pos) are unread, reads take the top ones.  Bits below 0 read as 0
// (pos going negative is an overrun the caller checks).
struct BitR {
  const uint8_t* s;
  uint32_t n;
  int64_t pos;
  int64_t wb;    // window: bytes [wb, wb + 8)
  uint64_t win;
  DSX_ZHD bool init(const uint8_t* src, uint32_t len) {
    s = src;
    n = len;
    wb = -1;
    win = 0;
    if (len == 0 || src[len - 1] == 0) return false;
    pos = 8 * (int64_t)(len - 1) + hibit(src[len - 1]);
    return true;
  }
  DSX_ZHD void load(int64_t b) {
    wb = b;
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) {
      const int64_t k = b + i;
      v = (v << 8) | (k < (int64_t)n ? s[k] : 0u);
    }
    win = v;
  }
  // bits [lo, lo + nb), nb <= 32
  DSX_ZHD uint32_t at(int64_t lo, int nb) {
    if (nb == 0) return 0;
    const int64_t hi = lo + nb;
    if (hi <= 0) return 0;
    int pad = 0;
    if (lo < 0) {
      pad = (int)-lo;
      lo = 0;
    }
    if (wb < 0 || lo < 8 * wb || hi > 8 * wb + 64) {
      const int64_t b = (hi + 7) / 8 - 8;
      load(b < 0 ? 0 : b);
    }
    const uint64_t v = (win >> (lo - 8 * wb)) & ((1ull << (nb - pad)) - 1ull);
    return (uint32_t)(v << pad);
  }
  DSX_ZHD uint32_t get(int nb) {
    pos -= nb;
    return at(pos, nb);
  }
  DSX_ZHD uint32_t peek(int nb) { return at(pos - nb, nb); }
};

// ---- FSE ---------------------------------------------------------------------------------------------------------
// Table description (forward bit stream) -> t.norm[0 .. *nsym); returns its bytes or -status.
DSX_ZHD inline int read_ncount(Tables& t, const uint8_t* s, uint32_t n, int max_sym, int max_log, int* log_out,
                               int* nsym_out) {
  if (n < 1) return -kErrTruncated;
  const int al = (s[0] & 15) + 5;
  if (al > max_log) return -kErrAccuracy;
  uint64_t bp = 4;
  auto rd = [&](int nb) -> uint32_t {
    uint32_t v = 0;
    for (int i = 0; i < nb; ++i) {
      const uint64_t q = bp + i;
      const uint32_t byte = (q >> 3) < n ? s[q >> 3] : 0u;
      v |= ((byte >> (q & 7)) & 1u) << i;
    }
    bp += nb;
    return v;
  };
  int remaining = 1 << al, sym = 0;
  while (remaining > 0) {
    if (sym > max_sym) return -kErrFse;
    const int bits = hibit((uint32_t)remaining + 1) + 1;
    uint32_t val = rd(bits);
    const uint32_t lower = (1u << (bits - 1)) - 1u;
    const uint32_t thr = (1u << bits) - 1u - ((uint32_t)remaining + 1u);
    if ((val & lower) < thr) {
      bp -= 1;
      val &= lower;
    } else if (val > lower) {
      val -= thr;
    }
    const int p = (int)val - 1;
    remaining -= p < 0 ? -p : p;
    t.norm[sym++] = (int16_t)p;
    if (p == 0) {
      uint32_t rep = rd(2);
      for (;;) {
        for (uint32_t i = 0; i < rep; ++i) {
          if (sym > max_sym) return -kErrFse;
          t.norm[sym++] = 0;
        }
        if (rep != 3) break;
        rep = rd(2);
      }
    }
    if ((bp + 7) / 8 > n) return -kErrTruncated;
  }
  if (remaining != 0) return -kErrFse;
  *log_out = al;
  *nsym_out = sym;
  return (int)((bp + 7) / 8);
}

// t.norm[0 .. nsym) of accuracy log al -> decoding table d (1 << al entries); returns a status
DSX_ZHD inline int build_fse(Tables& t, FseEntry* d, int nsym, int al) {
  const int size = 1 << al;
  int high = size;
  for (int s = 0; s < nsym; ++s)
    if (t.norm[s] == -1) {
      d[--high].sym = (uint8_t)s;
      t.sdesc[s] = 1;
    }
  const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  int pos = 0;
  for (int s = 0; s < nsym; ++s) {
    if (t.norm[s] <= 0) continue;
    t.sdesc[s] = (uint16_t)t.norm[s];
    for (int i = 0; i < t.norm[s]; ++i) {
      d[pos].sym = (uint8_t)s;
      do pos = (pos + step) & mask;
      while (pos >= high);
    }
  }
  if (pos != 0) return kErrFse;
  for (int i = 0; i < size; ++i) {
    const uint32_t nx = t.sdesc[d[i].sym]++;
    const int nb = al - hibit(nx);
    d[i].nb = (uint8_t)nb;
    d[i].base = (uint16_t)((nx << nb) - (uint32_t)size);
  }
  return kOk;
}

DSX_ZHD inline void rle_table(FseEntry* d, uint8_t sym) {
  d[0].sym = sym;
  d[0].nb = 0;
  d[0].base = 0;
}

// predefined distributions (RFC 8878 3.1.1.3.2.2), written as ranges: no constant arrays in device code (scratch)
// (predefined_norm / predefined_symbols / predefined_log are what the encoder of dsx_zstd_enc.h builds its tables from)
DSX_ZHD inline int predefined_symbols(int which) { return which == 0 ? 36 : (which == 1 ? 29 : 53); }  // 0 LL, 1 OF, 2 ML
DSX_ZHD inline int predefined_log(int which) { return which == 1 ? 5 : 6; }
DSX_ZHD inline int predefined_norm(int which, int i) {
  if (which == 0)
    return i == 0 ? 4 : i == 1 ? 3 : i < 13 ? 2 : i < 16 ? 1 : i < 25 ? 2 : i == 25 ? 3 : i == 26 ? 2 : i < 32 ? 1 : -1;
  if (which == 1) return i < 6 ? 1 : i < 9 ? 2 : i < 24 ? 1 : -1;
  return i == 0 ? 1 : i == 1 ? 4 : i == 2 ? 3 : i < 9 ? 2 : i < 46 ? 1 : -1;
}
DSX_ZHD inline int predefined(Tables& t, int which) {  // 0 LL, 1 OF, 2 ML; returns nsym
  const int nsym = predefined_symbols(which);
  for (int i = 0; i < nsym; ++i) t.norm[i] = (int16_t)predefined_norm(which, i);
  return nsym;
}

// ---- Huffman -----------------------------------------------------------------------------------------------------
// Tree description at s (n bytes available) -> t.huf / t.huf_log; returns its bytes or -status.
DSX_ZHD inline int read_huf_tree(Tables& t, const uint8_t* s, uint32_t n) {
  if (n < 1) return -kErrTruncated;
  const int hb = s[0];
  int nw = 0, used = 0;
  if (hb < 128) {  // FSE-compressed weights, hb bytes
    if (hb == 0) return -kErrHuffman;
    if ((uint32_t)hb + 1 > n) return -kErrTruncated;
    const uint8_t* f = s + 1;
    int al = 0, nsym = 0;
    const int hdr = read_ncount(t, f, (uint32_t)hb, 15, kLogWt, &al, &nsym);
    if (hdr < 0) return hdr;
    const int st = build_fse(t, t.wt, nsym, al);
    if (st) return -st;
    BitR r;
    if (!r.init(f + hdr, (uint32_t)(hb - hdr))) return -kErrBitstream;
    uint32_t s1 = r.get(al), s2 = r.get(al);
    if (r.pos < 0) return -kErrBitstream;
    for (;;) {
      if (nw > 255 - 2) return -kErrHuffman;
      t.w[nw++] = t.wt[s1].sym;
      s1 = t.wt[s1].base + r.get(t.wt[s1].nb);
      if (r.pos < 0) {
        t.w[nw++] = t.wt[s2].sym;
        break;
      }
      t.w[nw++] = t.wt[s2].sym;
      s2 = t.wt[s2].base + r.get(t.wt[s2].nb);
      if (r.pos < 0) {
        t.w[nw++] = t.wt[s1].sym;
        break;
      }
    }
    used = 1 + hb;
  } else {  // direct: 4 bits per weight
    nw = hb - 127;
    const int bytes = (nw + 1) / 2;
    if ((uint32_t)bytes + 1 > n) return -kErrTruncated;
    for (int i = 0; i < nw; ++i) t.w[i] = (uint8_t)((i & 1) ? (s[1 + i / 2] & 15) : (s[1 + i / 2] >> 4));
    used = 1 + bytes;
  }
  uint32_t total = 0;
  for (int i = 0; i < nw; ++i) {
    if (t.w[i] > kHufMaxBits) return -kErrHuffman;
    total += t.w[i] ? (1u << (t.w[i] - 1)) : 0u;
  }
  if (total == 0) return -kErrHuffman;
  const int mb = hibit(total) + 1;
  if (mb > kHufMaxBits) return -kErrHuffman;
  const uint32_t left = (1u << mb) - total;
  if (left == 0 || (left & (left - 1))) return -kErrHuffman;
  t.w[nw] = (uint8_t)(hibit(left) + 1);
  const int nsym = nw + 1;
  // weights -> code lengths (in place), rank counts, then the table: the longest codes first
  for (int l = 0; l <= kHufMaxBits + 1; ++l) t.rank[l] = 0;
  for (int i = 0; i < nsym; ++i) {
    t.w[i] = t.w[i] ? (uint8_t)(mb + 1 - t.w[i]) : 0;
    t.rank[t.w[i]]++;
  }
  uint32_t idx = 0;
  for (int l = mb; l >= 1; --l) {  // rank[l]: count -> first table index of the codes of length l
    const uint32_t span = (uint32_t)t.rank[l] << (mb - l);
    t.rank[l] = (uint16_t)idx;
    for (uint32_t k = 0; k < span; ++k) t.huf[idx + k].nb = (uint8_t)l;
    idx += span;
  }
  for (int i = 0; i < nsym; ++i) {
    const int l = t.w[i];
    if (!l) continue;
    const uint32_t span = 1u << (mb - l);
    for (uint32_t k = 0; k < span; ++k) t.huf[t.rank[l] + k].sym = (uint8_t)i;
    t.rank[l] = (uint16_t)(t.rank[l] + span);
  }
  t.huf_log = mb;
  return used;
}

// One Huffman stream of `cnt` symbols -> dst; returns a status
DSX_ZHD inline int huf_stream(const Tables& t, const uint8_t* s, uint32_t n, uint8_t* dst, uint32_t cnt) {
  BitR r;
  if (!r.init(s, n)) return kErrBitstream;
  const int log = t.huf_log;
  for (uint32_t i = 0; i < cnt; ++i) {
    const HufEntry e = t.huf[r.peek(log)];
    dst[i] = e.sym;
    r.pos -= e.nb;
    if (r.pos < 0) return kErrBitstream;
  }
  return r.pos == 0 ? kOk : kErrBitstream;
}

// ---- frame and block headers -------------------------------------------------------------------------------------
struct FrameHdr {
  uint32_t bytes;      // header bytes
  int64_t content;     // Frame_Content_Size, -1 if absent
  int checksum, dict;
};

// Returns a status; fills h.  Frames with a dictionary ID or a checksum are kErrUnsupported.
DSX_ZHD inline int frame_header(const uint8_t* s, uint32_t n, FrameHdr& h) {
  if (n < 5) return kErrTruncated;
  if (le(s, 4) != kMagic) return kErrMagic;
  const uint32_t d = s[4];
  const int fcs_flag = (int)(d >> 6), single = (int)((d >> 5) & 1), dict_flag = (int)(d & 3);
  h.checksum = (int)((d >> 2) & 1);
  h.dict = dict_flag != 0;
  if (d & 0x08) return kErrReserved;
  uint32_t p = 5;
  if (!single) ++p;  // window descriptor (the output size bounds every offset here)
  const int did_bytes = dict_flag == 0 ? 0 : (dict_flag == 1 ? 1 : (dict_flag == 2 ? 2 : 4));
  p += (uint32_t)did_bytes;
  const int fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : (fcs_flag == 1 ? 2 : (fcs_flag == 2 ? 4 : 8));
  if (p + (uint32_t)fcs_bytes > n) return kErrTruncated;
  h.content = -1;
  if (fcs_bytes == 1) h.content = s[p];
  else if (fcs_bytes == 2) h.content = (int64_t)le(s + p, 2) + 256;
  else if (fcs_bytes == 4) h.content = (int64_t)le(s + p, 4);
  else if (fcs_bytes == 8) h.content = (int64_t)(((uint64_t)le(s + p + 4, 4) << 32) | le(s + p, 4));
  if (h.content < 0 && fcs_bytes == 8) h.content = INT64_MAX;
  h.bytes = p + (uint32_t)fcs_bytes;
  if (h.dict || h.checksum) return kErrUnsupported;
  return kOk;
}

// Whether a zstd frame of a Blosc block of `want` bytes is for the device: its descriptor names no dictionary and no
// checksum, and a content size, if present, is `want`.  (Anything else -- a malformed frame included -- is left to
// the decoder, which reports it.)
DSX_ZHD inline bool device_frame(const uint8_t* s, uint32_t n, uint32_t want) {
  FrameHdr h;
  const int st = frame_header(s, n, h);
  if (st == kErrUnsupported) return false;
  if (st == kOk && h.content >= 0 && h.content != (int64_t)want) return false;
  return true;
}

// Literals section of a compressed block: where the literals are and how they are coded
struct LitHdr {
  int type;              // 0 raw, 1 RLE, 2 compressed, 3 treeless
  int streams;           // 1 or 4 (compressed / treeless)
  uint32_t hdr;          // header bytes
  uint32_t regen;        // literals
  uint32_t csize;        // bytes after the header (raw: regen, RLE: 1, compressed: tree + jump table + streams)
};

DSX_ZHD inline int lit_header(const uint8_t* s, uint32_t n, LitHdr& h) {
  if (n < 1) return kErrTruncated;
  const uint32_t b0 = s[0];
  h.type = (int)(b0 & 3);
  const int sf = (int)((b0 >> 2) & 3);
  h.streams = 1;
  if (h.type < 2) {
    if (sf == 0 || sf == 2) { h.hdr = 1; h.regen = b0 >> 3; }
    else if (sf == 1) { if (n < 2) return kErrTruncated; h.hdr = 2; h.regen = (b0 >> 4) + ((uint32_t)s[1] << 4); }
    else { if (n < 3) return kErrTruncated; h.hdr = 3; h.regen = (b0 >> 4) + ((uint32_t)s[1] << 4) + ((uint32_t)s[2] << 12); }
    h.csize = h.type == 0 ? h.regen : 1;
  } else {
    h.streams = sf == 0 ? 1 : 4;
    if (sf < 2) {
      if (n < 3) return kErrTruncated;
      const uint32_t v = le(s, 3);
      h.hdr = 3; h.regen = (v >> 4) & 0x3FF; h.csize = (v >> 14) & 0x3FF;
    } else if (sf == 2) {
      if (n < 4) return kErrTruncated;
      const uint32_t v = le(s, 4);
      h.hdr = 4; h.regen = (v >> 4) & 0x3FFF; h.csize = (v >> 18) & 0x3FFF;
    } else {
      if (n < 5) return kErrTruncated;
      const uint64_t v = (uint64_t)le(s, 4) | ((uint64_t)s[4] << 32);
      h.hdr = 5; h.regen = (uint32_t)((v >> 4) & 0x3FFFF); h.csize = (uint32_t)((v >> 22) & 0x3FFFF);
    }
  }
  if (h.regen > kBlockMax) return kErrLiterals;
  if (h.hdr + h.csize > n) return kErrTruncated;
  return kOk;
}

// Stream k of a 4-stream literal section (after the tree): offset / bytes within the section, and its symbols
struct Streams {
  uint32_t off[4], len[4], cnt[4];
};
DSX_ZHD inline int split_streams(const uint8_t* s, uint32_t n, uint32_t regen, int streams, Streams& st) {
  if (streams == 1) {
    st.off[0] = 0; st.len[0] = n; st.cnt[0] = regen;
    for (int k = 1; k < 4; ++k) { st.off[k] = n; st.len[k] = 0; st.cnt[k] = 0; }
    return kOk;
  }
  if (n < 6) return kErrTruncated;
  const uint32_t l0 = le(s, 2), l1 = le(s + 2, 2), l2 = le(s + 4, 2);
  if (6ull + l0 + l1 + l2 > n) return kErrLiterals;
  const uint32_t seg = (regen + 3) / 4;
  if (3 * seg > regen) return kErrLiterals;
  st.off[0] = 6; st.len[0] = l0;
  st.off[1] = 6 + l0; st.len[1] = l1;
  st.off[2] = 6 + l0 + l1; st.len[2] = l2;
  st.off[3] = 6 + l0 + l1 + l2; st.len[3] = n - st.off[3];
  for (int k = 0; k < 3; ++k) st.cnt[k] = seg;
  st.cnt[3] = regen - 3 * seg;
  return kOk;
}

// ---- sequences ---------------------------------------------------------------------------------------------------
// baselines and extra bits of the length codes (RFC 8878 3.1.1.3.2.1.1), as formulas
DSX_ZHD inline uint32_t ll_base(int c) {
  if (c < 16) return (uint32_t)c;
  if (c < 20) return 16u + 2u * (uint32_t)(c - 16);
  if (c < 22) return 24u + 4u * (uint32_t)(c - 20);
  if (c < 24) return 32u + 8u * (uint32_t)(c - 22);
  if (c == 24) return 48u;
  return 1u << (c - 19);
}
DSX_ZHD inline int ll_bits(int c) {
  return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c - 19;
}
DSX_ZHD inline uint32_t ml_base(int c) {
  if (c < 32) return (uint32_t)c + 3u;
  if (c < 36) return 35u + 2u * (uint32_t)(c - 32);
  if (c < 38) return 43u + 4u * (uint32_t)(c - 36);
  if (c < 40) return 51u + 8u * (uint32_t)(c - 38);
  if (c < 42) return 67u + 16u * (uint32_t)(c - 40);
  if (c == 42) return 99u;
  return (1u << (c - 36)) + 3u;
}
DSX_ZHD inline int ml_bits(int c) {
  return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36;
}

// One of the three tables of a sequences section at s; returns its bytes or -status
DSX_ZHD inline int seq_table(Tables& t, int which, int mode, const uint8_t* s, uint32_t n) {
  FseEntry* d = which == 0 ? t.ll : (which == 1 ? t.of : t.ml);
  int* lg = which == 0 ? &t.ll_log : (which == 1 ? &t.of_log : &t.ml_log);
  const int max_sym = which == 0 ? kMaxLL : (which == 1 ? kMaxOF : kMaxML);
  const int max_log = which == 0 ? kLogLL : (which == 1 ? kLogOF : kLogML);
  if (mode == 0) {
    const int nsym = predefined(t, which);
    const int al = predefined_log(which);
    const int st = build_fse(t, d, nsym, al);
    if (st) return -st;
    *lg = al;
    return 0;
  }
  if (mode == 1) {
    if (n < 1) return -kErrTruncated;
    if (s[0] > max_sym) return -kErrSequences;
    rle_table(d, s[0]);
    *lg = 0;
    return 1;
  }
  if (mode == 2) {
    int al = 0, nsym = 0;
    const int used = read_ncount(t, s, n, max_sym, max_log, &al, &nsym);
    if (used < 0) return used;
    const int st = build_fse(t, d, nsym, al);
    if (st) return -st;
    *lg = al;
    return used;
  }
  return *lg < 0 ? -kErrSequences : 0;  // repeat: the previous table of the frame
}

struct Seq {
  uint32_t ll, ml, off;
};

// Decoder state of the sequences of one block (registers)
struct SeqState {
  BitR r;
  uint32_t sll, sof, sml;       // FSE states
  uint32_t rep0, rep1, rep2;    // repeat offsets (frame lifetime)
  uint32_t op;                  // output written once the decoded sequences are executed
  uint32_t lit_used, nlit;      // literals of the block consumed / present
  uint32_t left;                // sequences still to decode
};

// Sequences section header + tables at s (n bytes: the rest of the block); st.r starts the bitstream.  Returns a
// status; *nseq = 0 when the block has no sequences.
DSX_ZHD inline int seq_header(Tables& t, const uint8_t* s, uint32_t n, SeqState& st, uint32_t* nseq) {
  if (n < 1) return kErrTruncated;
  uint32_t p;
  const uint32_t b0 = s[0];
  if (b0 == 0) {
    *nseq = 0;
    return n == 1 ? kOk : kErrBitstream;
  }
  if (b0 < 128) { *nseq = b0; p = 1; }
  else if (b0 < 255) { if (n < 2) return kErrTruncated; *nseq = ((b0 - 128) << 8) + s[1]; p = 2; }
  else { if (n < 3) return kErrTruncated; *nseq = s[1] + ((uint32_t)s[2] << 8) + 0x7F00; p = 3; }
  if (p >= n) return kErrTruncated;
  const uint32_t modes = s[p++];
  if (modes & 3) return kErrReserved;
  for (int k = 0; k < 3; ++k) {  // LL, OF, ML
    const int used = seq_table(t, k, (int)((modes >> (6 - 2 * k)) & 3), s + p, n - p);
    if (used < 0) return -used;
    p += (uint32_t)used;
  }
  if (!st.r.init(s + p, n - p)) return kErrBitstream;
  st.sll = st.r.get(t.ll_log);
  st.sof = st.r.get(t.of_log);
  st.sml = st.r.get(t.ml_log);
  if (st.r.pos < 0) return kErrBitstream;
  st.left = *nseq;
  return kOk;
}

// Next sequence, validated against the literals and the output (out_n bytes): returns a status.  Updates op and
// lit_used as if the sequence had been executed.
DSX_ZHD inline int next_seq(const Tables& t, SeqState& st, uint32_t out_n, Seq& q) {
  const FseEntry el = t.ll[st.sll], eo = t.of[st.sof], em = t.ml[st.sml];
  const int ofc = eo.sym, mlc = em.sym, llc = el.sym;
  if (ofc > kMaxOF || mlc > kMaxML || llc > kMaxLL) return kErrSequences;
  const uint32_t ofv = (1u << ofc) + st.r.get(ofc);
  const uint32_t ml = ml_base(mlc) + st.r.get(ml_bits(mlc));
  const uint32_t ll = ll_base(llc) + st.r.get(ll_bits(llc));
  st.left--;
  if (st.left) {
    st.sll = el.base + st.r.get(el.nb);
    st.sml = em.base + st.r.get(em.nb);
    st.sof = eo.base + st.r.get(eo.nb);
  }
  if (st.r.pos < 0) return kErrBitstream;
  uint32_t off;
  if (ofv > 3) {
    off = ofv - 3;
    st.rep2 = st.rep1; st.rep1 = st.rep0; st.rep0 = off;
  } else {
    const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
    if (idx == 0) {
      off = st.rep0;
    } else {
      off = idx == 1 ? st.rep1 : (idx == 2 ? st.rep2 : st.rep0 - 1);
      if (idx > 1) st.rep2 = st.rep1;
      st.rep1 = st.rep0;
      st.rep0 = off;
    }
  }
  if (ll > st.nlit - st.lit_used) return kErrSequences;
  st.lit_used += ll;
  const uint32_t at = st.op + ll;
  if (off == 0 || off > at) return kErrOffset;
  if (ml > out_n - at || ll > out_n - st.op) return kErrOutput;
  st.op = at + ml;
  q.ll = ll;
  q.ml = ml;
  q.off = off;
  return kOk;
}

// End of a block's sequences: the bitstream consumed exactly
DSX_ZHD inline int seq_end(const SeqState& st) { return st.r.pos == 0 ? kOk : kErrBitstream; }

// ---- host build: one whole frame ---------------------------------------------------------------------------------
// Frame s[0 .. n) -> out[0 .. out_n), exactly.  t: the caller's work space.
inline int decode_frame(Tables& t, const uint8_t* s, uint32_t n, uint8_t* out, uint32_t out_n) {
  FrameHdr fh;
  int st = frame_header(s, n, fh);
  if (st) return st;
  if (fh.content >= 0 && fh.content != (int64_t)out_n) return kErrOutput;
  t.huf_log = 0;
  t.ll_log = t.of_log = t.ml_log = -1;
  SeqState q;
  q.rep0 = 1; q.rep1 = 4; q.rep2 = 8;
  uint32_t ip = fh.bytes, op = 0;
  for (;;) {
    if (n - ip < 3) return kErrTruncated;
    const uint32_t bh = le(s + ip, 3);
    ip += 3;
    const int last = (int)(bh & 1), type = (int)((bh >> 1) & 3);
    const uint32_t bs = bh >> 3;
    if (type == 3) return kErrReserved;
    if (bs > kBlockMax) return kErrBlockSize;
    if (type == 0) {
      if (bs > n - ip) return kErrTruncated;
      if (bs > out_n - op) return kErrOutput;
      copy_bytes(out + op, s + ip, bs);
      ip += bs;
      op += bs;
    } else if (type == 1) {
      if (n - ip < 1) return kErrTruncated;
      if (bs > out_n - op) return kErrOutput;
      for (uint32_t i = 0; i < bs; ++i) out[op + i] = s[ip];
      ip += 1;
      op += bs;
    } else {
      if (bs > n - ip) return kErrTruncated;
      const uint8_t* b = s + ip;
      LitHdr lh;
      st = lit_header(b, bs, lh);
      if (st) return st;
      if (lh.regen > out_n - op) return kErrOutput;
      const uint8_t* lit;
      uint8_t* lit_dst = out + (out_n - lh.regen);
      if (lh.type == 0) {
        lit = b + lh.hdr;
      } else if (lh.type == 1) {
        for (uint32_t i = 0; i < lh.regen; ++i) lit_dst[i] = b[lh.hdr];
        lit = lit_dst;
      } else {
        uint32_t tree = 0;
        if (lh.type == 2) {
          const int used = read_huf_tree(t, b + lh.hdr, lh.csize);
          if (used < 0) return -used;
          tree = (uint32_t)used;
        } else if (t.huf_log == 0) {
          return kErrHuffman;
        }
        Streams ss;
        const uint8_t* sb = b + lh.hdr + tree;
        st = split_streams(sb, lh.csize - tree, lh.regen, lh.streams, ss);
        if (st) return st;
        uint32_t at = 0;
        for (int k = 0; k < lh.streams; ++k) {
          st = huf_stream(t, sb + ss.off[k], ss.len[k], lit_dst + at, ss.cnt[k]);
          if (st) return st;
          at += ss.cnt[k];
        }
        lit = lit_dst;
      }
      const uint32_t sp = lh.hdr + lh.csize;
      uint32_t nseq = 0;
      q.op = op;
      q.lit_used = 0;
      q.nlit = lh.regen;
      st = seq_header(t, b + sp, bs - sp, q, &nseq);
      if (st) return st;
      for (uint32_t k = 0; k < nseq; ++k) {
        Seq e;
        const uint32_t o0 = q.op, l0 = q.lit_used;
        st = next_seq(t, q, out_n, e);
        if (st) return st;
        run_seq_host(out + o0, lit + l0, e.ll, e.ml, e.off);
      }
      if (nseq) {
        st = seq_end(q);
        if (st) return st;
      }
      const uint32_t rest = lh.regen - q.lit_used;
      if (rest > out_n - q.op) return kErrOutput;
      copy_bytes(out + q.op, lit + q.lit_used, rest);  // (from above, when the literals lie at the end of out)
      if (q.op + rest - op > kBlockMax) return kErrBlockSize;
      op = q.op + rest;
      ip += bs;
    }
    if (last) break;
  }
  if (op != out_n) return kErrOutput;
  if (ip != n) return kErrTruncated;
  return kOk;
}

}  // namespace zdec
}  // namespace dsx

#endif  // DSX_ZSTD_DEC_H
