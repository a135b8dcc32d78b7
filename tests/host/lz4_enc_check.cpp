// Host build of the Blosc-LZ4 encoder (csrc/dsx_lz4_enc.h), for tests/test_lz4_encoder_host.py:
//   lz4_enc_check <chunks.raw> <chunk_bytes> <clevel> <frames.out> <offsets.out> [<chunks>]
// encodes the uint16 chunks of <chunks.raw> (back to back) and writes the packed frames and the n + 1 int64 offsets;
// <chunks>: how many chunks of 0 bytes there are (a file does not say).
// The frame buffer is exactly n * (chunk_bytes + 16) bytes, so a sanitizer build sees a frame that outgrows its bound.
//   lz4_enc_check --stream <bytes.in> <block.out>
// encodes the bytes of <bytes.in> as one stream (encode_stream_host, into a buffer of the stream's own length) and
// writes the LZ4 block; an empty file when the stream is stored.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_lz4_enc.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_file(const char* path, std::vector<uint8_t>& raw) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  static uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  return true;
}

static int one_stream(const char* in, const char* out) {
  std::vector<uint8_t> raw;
  if (!read_file(in, raw)) return 2;
  std::vector<uint8_t> block(raw.size());
  std::vector<uint32_t> table(dsx::lz4enc::kTable);
  const uint32_t n = dsx::lz4enc::encode_stream_host(raw.data(), (uint32_t)raw.size(), block.data(), table.data());
  FILE* o = fopen(out, "wb");
  if (!o || fwrite(block.data(), 1, n, o) != n) return 3;
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--stream")) return one_stream(argv[2], argv[3]);
  if (argc != 6 && argc != 7) {
    fprintf(stderr, "usage: %s chunks.raw chunk_bytes clevel frames.out offsets.out | --stream bytes.in block.out\n", argv[0]);
    return 2;
  }
  std::vector<uint8_t> raw;
  if (!read_file(argv[1], raw)) return 2;
  const uint64_t chunk = strtoull(argv[2], nullptr, 10);
  const int clevel = atoi(argv[3]);
  if (chunk % 2 || (chunk && raw.size() % chunk)) { fprintf(stderr, "bad chunk size\n"); return 2; }
  const uint64_t n = chunk ? raw.size() / chunk : (argc == 7 ? strtoull(argv[6], nullptr, 10) : 0);
  std::vector<uint8_t> frames(n * (chunk + 16));
  std::vector<int64_t> offsets(n + 1);
  std::vector<uint16_t> src(raw.size() / 2);
  for (size_t i = 0; i + 1 < raw.size(); i += 2) src[i / 2] = (uint16_t)(raw[i] | (raw[i + 1] << 8));
  dsx::lz4enc::blosc_encode_host(src.data(), n, chunk, clevel, frames.data(), offsets.data());
  FILE* o = fopen(argv[4], "wb");
  if (!o || fwrite(frames.data(), 1, (size_t)offsets[n], o) != (size_t)offsets[n]) return 3;
  fclose(o);
  o = fopen(argv[5], "wb");
  if (!o || fwrite(offsets.data(), 8, n + 1, o) != n + 1) return 3;
  fclose(o);
  return 0;
}
