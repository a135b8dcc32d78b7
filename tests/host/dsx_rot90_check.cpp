// Host check of csrc/dsx_rot90.h (no GPU): the blocks of rot_grid, walked element by element as k_rot90 walks them
// (rot_elem for tile positions [0, 64) x [0, 64) of every block), must write every destination element of every shape
// exactly once, from the source element np.rot90 names, and never index outside a plane or the LDS tile; the grid must
// cover the partial tiles of both axes with no block that is wholly outside.  Prints one JSON object.
//
//   g++ -std=c++17 -O2 -o dsx_rot90_check tests/host/dsx_rot90_check.cpp        (or with -fsanitize=address,undefined)
#include <stdio.h>

#include <vector>

#include "../../aind_smartspim_destripe_amd/csrc/dsx_rot90.h"

using namespace dsx::rot;

static const int kShapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 5}, {63, 65}, {64, 64}, {65, 63}, {70, 100}, {129, 257}};

template <typename T>
static bool check_shape(int n, int H, int W, int dir, long long* checked) {
  const size_t px = (size_t)H * W;
  std::vector<T> src(px * n), want(px * n), got(px * n, (T)0);
  for (size_t k = 0; k < src.size(); ++k) src[k] = (T)(k % 65521u + 1u);
  rot90_host(src.data(), want.data(), n, H, W, dir);
  std::vector<int> writes(px * n, 0);
  std::vector<T> tile((size_t)kRotTile * rot_pitch(sizeof(T)));
  if (rot_lds_bytes(sizeof(T)) != tile.size() * sizeof(T)) return false;
  const RotGrid g = rot_grid(n, H, W);
  // partial tiles are covered, and no block lies wholly outside the plane
  if ((long long)g.x * kRotTile < W || (long long)(g.x - 1) * kRotTile >= W) return false;
  if ((long long)g.y * kRotTile < H || (long long)(g.y - 1) * kRotTile >= H) return false;
  if (g.z != (unsigned)n) return false;
  const int P = rot_pitch(sizeof(T));
  for (unsigned bz = 0; bz < g.z; ++bz)
    for (unsigned by = 0; by < g.y; ++by)
      for (unsigned bx = 0; bx < g.x; ++bx) {
        // phase 1: the tile from the source, [tj][tc]
        for (int tj = 0; tj < kRotTile; ++tj)
          for (int tc = 0; tc < kRotTile; ++tc) {
            const RotElem e = rot_elem(dir, H, W, bx, by, tj, tc);
            if (!e.live) continue;
            if (e.src >= px) return false;
            tile.at((size_t)tj * P + tc) = src[bz * px + e.src];
          }
        // phase 2: the destination from the tile, read down its columns
        for (int tc = 0; tc < kRotTile; ++tc)
          for (int tj = 0; tj < kRotTile; ++tj) {
            const RotElem e = rot_elem(dir, H, W, bx, by, tj, tc);
            if (!e.live) continue;
            if (e.dst >= px) return false;
            got[bz * px + e.dst] = tile.at((size_t)tj * P + tc);
            ++writes[bz * px + e.dst];
            ++*checked;
          }
      }
  for (size_t k = 0; k < writes.size(); ++k)
    if (writes[k] != 1 || got[k] != want[k]) return false;
  // the map itself against its definition: np.rot90(x)[i, j] == x[j, W - 1 - i]; np.rot90(x, -1)[i, j] == x[H - 1 - j, i]
  for (int i = 0; i < W; ++i)
    for (int j = 0; j < H; ++j) {
      const size_t s = dir > 0 ? (size_t)j * W + (W - 1 - i) : (size_t)(H - 1 - j) * W + i;
      if (want[(size_t)i * H + j] != src[s]) return false;
    }
  return true;
}

// the transposed LDS read of phase 2: the 32 lanes of a group (tile rows k .. k + 31 of one tile column) on 32 banks
static bool check_banks(size_t elem_bytes) {
  const int P = rot_pitch(elem_bytes);
  for (int tc = 0; tc < kRotTile; ++tc)
    for (int half = 0; half < 2; ++half) {
      bool seen[32] = {};
      for (int k = 0; k < 32; ++k) {
        const size_t byte = ((size_t)(half * 32 + k) * P + tc) * elem_bytes;
        const int bank = (int)((byte / 4) % 32);
        if (seen[bank]) return false;
        seen[bank] = true;
      }
    }
  return true;
}

int main() {
  long long checked = 0;
  bool ok = check_banks(2) && check_banks(4);
  for (const auto& s : kShapes)
    for (int n : {1, 3})
      for (int dir : {1, -1}) {
        ok = ok && check_shape<uint16_t>(n, s[0], s[1], dir, &checked);
        ok = ok && check_shape<float>(n, s[0], s[1], dir, &checked);
      }
  // the round trip is the identity
  {
    const int H = 70, W = 100;
    std::vector<uint16_t> a((size_t)H * W), b(a.size()), c(a.size());
    for (size_t k = 0; k < a.size(); ++k) a[k] = (uint16_t)(k * 7u);
    rot90_host(a.data(), b.data(), 1, H, W, 1);
    rot90_host(b.data(), c.data(), 1, W, H, -1);
    ok = ok && a == c;
  }
  printf("{\"ok\": %s, \"checked\": %lld}\n", ok ? "true" : "false", checked);
  return ok ? 0 : 1;
}
