// Host build of the device Blosc-zstd encoder with its mode (csrc/dsx_zstd_enc.h), for
// tests/test_zstd_encoder_runs_host.py:
//   zstd_enc_runs_check <chunks.raw> <chunk_bytes> <clevel> <mode> <frames.out> <offsets.out> [<chunks>]
// encodes the uint16 chunks of <chunks.raw> (back to back) and writes the packed frames and the n + 1 int64 offsets.
// <chunks>: how many chunks of 0 bytes there are (a file does not say).
//   zstd_enc_runs_check --codes
// checks the length-code formulas of the encoder against the baselines of the decoder, for every length of a block.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_zstd_enc.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int check_codes() {
  namespace d = dsx::zdec;
  namespace e = dsx::zenc;
  for (uint32_t v = 0; v < 131072; ++v) {  // (a block with a match has fewer literals than bytes)
    const int c = e::ll_code(v);
    if (c < 0 || c > d::kMaxLL || v < d::ll_base(c) || v - d::ll_base(c) >= (1u << d::ll_bits(c))) {
      fprintf(stderr, "literal length %u: code %d\n", v, c);
      return 1;
    }
  }
  for (uint32_t v = 3; v <= 131072; ++v) {
    const int c = e::ml_code(v);
    if (c < 0 || c > d::kMaxML || v < d::ml_base(c) || v - d::ml_base(c) >= (1u << d::ml_bits(c))) {
      fprintf(stderr, "match length %u: code %d\n", v, c);
      return 1;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--codes")) return check_codes();
  if (argc != 7 && argc != 8) {
    fprintf(stderr, "usage: %s chunks.raw chunk_bytes clevel mode frames.out offsets.out | --codes\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> raw;
  static uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  const uint64_t chunk = strtoull(argv[2], nullptr, 10);
  const int clevel = atoi(argv[3]), mode = atoi(argv[4]);
  if (chunk % 2 || (chunk && raw.size() % chunk)) { fprintf(stderr, "bad chunk size\n"); return 2; }
  const uint64_t n = chunk ? raw.size() / chunk : (argc == 8 ? strtoull(argv[7], nullptr, 10) : 0);
  std::vector<uint8_t> frames(n * (chunk + 16) + 1);
  std::vector<int64_t> offsets(n + 1);
  std::vector<uint16_t> src(raw.size() / 2 + 1);
  for (size_t i = 0; i + 1 < raw.size(); i += 2) src[i / 2] = (uint16_t)(raw[i] | (raw[i + 1] << 8));
  dsx::zenc::blosc_encode_host(src.data(), n, chunk, clevel, frames.data(), offsets.data(), mode);
  FILE* o = fopen(argv[5], "wb");
  if (!o || fwrite(frames.data(), 1, (size_t)offsets[n], o) != (size_t)offsets[n]) return 3;
  fclose(o);
  o = fopen(argv[6], "wb");
  if (!o || fwrite(offsets.data(), 8, n + 1, o) != n + 1) return 3;
  fclose(o);
  return 0;
}
