// Host build of the device Blosc-zstd encoder (csrc/dsx_zstd_enc.h), for tests/test_zstd_encoder_host.py:
//   zstd_enc_check <chunks.raw> <chunk_bytes> <clevel> <frames.out> <offsets.out> [<chunks>]
// encodes the uint16 chunks of <chunks.raw> (back to back) and writes the packed frames and the n + 1 int64 offsets.
// <chunks>: how many chunks of 0 bytes there are (a file does not say).
#include "../../aind_smartspim_destripe_amd/csrc/dsx_zstd_enc.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) {
    fprintf(stderr, "usage: %s chunks.raw chunk_bytes clevel frames.out offsets.out [chunks]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> raw;
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  const uint64_t chunk = strtoull(argv[2], nullptr, 10);
  const int clevel = atoi(argv[3]);
  if (chunk % 2 || (chunk && raw.size() % chunk)) { fprintf(stderr, "bad chunk size\n"); return 2; }
  const uint64_t n = chunk ? raw.size() / chunk : (argc == 7 ? strtoull(argv[6], nullptr, 10) : 0);
  std::vector<uint8_t> frames(n * (chunk + 16) + 1);
  std::vector<int64_t> offsets(n + 1);
  std::vector<uint16_t> src(raw.size() / 2 + 1);
  for (size_t i = 0; i + 1 < raw.size(); i += 2) src[i / 2] = (uint16_t)(raw[i] | (raw[i + 1] << 8));
  dsx::zenc::blosc_encode_host(src.data(), n, chunk, clevel, frames.data(), offsets.data());
  FILE* o = fopen(argv[4], "wb");
  if (!o || fwrite(frames.data(), 1, (size_t)offsets[n], o) != (size_t)offsets[n]) return 3;
  fclose(o);
  o = fopen(argv[5], "wb");
  if (!o || fwrite(offsets.data(), 8, n + 1, o) != n + 1) return 3;
  fclose(o);
  return 0;
}
