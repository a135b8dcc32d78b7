// Host-side (g++) checks of what k_rowfilter_pack takes from dsx_chain.h: the map from a wave's virtual butterfly index to
// (row pair, butterfly), the pack factor per level and its two bounds, and the launch geometry.  For the transform lengths
// of the coarse levels of a 2048^2 plane (260, 132, 144, 36, 20, 12) and 1 ... 4 row pairs per wave.  Prints one JSON
// object; exit status 1 when a check fails (tests/test_row_pack_host.py).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../aind_smartspim_destripe_amd/csrc/dsx_plan.h"
#include "../../aind_smartspim_destripe_amd/csrc/dsx_chain.h"

static long long g_checked = 0;
static int g_failed = 0;

#define CHECK(cond, ...)                         \
  do {                                           \
    ++g_checked;                                 \
    if (!(cond)) {                               \
      if (g_failed++ < 20) {                     \
        fprintf(stderr, "FAILED %s: ", #cond);   \
        fprintf(stderr, __VA_ARGS__);            \
        fprintf(stderr, "\n");                   \
      }                                          \
    }                                            \
  } while (0)

struct Length {
  int M;
  int npass;
  int radix[4];   // the plan's pass list (dsx::factorize)
  int best;       // pack factor of least modelled cost
  int cost1;      // modelled cost per pair, one pair per wave (to the nearest integer, +- 0.5)
  int cost_best;  // ... at the best pack factor
  int npairs;     // row pairs of the level in a 2048^2 plane
};
static const Length kLengths[6] = {
    {260, 3, {13, 5, 4}, 3, 630, 309, 130}, {132, 3, {11, 3, 4}, 4, 472, 168, 66}, {144, 3, {6, 6, 4}, 4, 408, 175, 34},
    {36, 2, {6, 6}, 4, 284, 71, 18},        {20, 2, {5, 4}, 4, 268, 67, 10},       {12, 2, {3, 4}, 4, 221, 55, 6},
};

// what the lanes of a wave visit in one joint pass: MAXB rounds of 64 virtual butterflies
static void check_map(int M, int n, int rounds, int P, int nlive) {
  std::vector<int> seen((size_t)nlive * n, 0);
  const int total = nlive * n;
  for (int i = 0; i < rounds; ++i) {
    for (int lane = 0; lane < 64; ++lane) {
      const int v = lane + 64 * i;
      if (v >= total) continue;
      int off, b, p1, b1;
      dsx::row_pack_split(v, n, M, off, b);
      dsx::row_pack_split(v, n, 1, p1, b1);
      CHECK(off == p1 * M && b == b1, "M=%d n=%d v=%d", M, n, v);
      CHECK(p1 >= 0 && p1 < nlive && b >= 0 && b < n, "M=%d n=%d v=%d -> (%d, %d), %d live", M, n, v, p1, b, nlive);
      CHECK(p1 == v / n && b == v % n, "M=%d n=%d v=%d -> (%d, %d)", M, n, v, p1, b);
      if (p1 >= 0 && p1 < nlive && b >= 0 && b < n) ++seen[(size_t)p1 * n + b];
    }
  }
  for (int k = 0; k < total; ++k) CHECK(seen[k] == 1, "M=%d n=%d P=%d live=%d: (%d, %d) visited %d times", M, n, P, nlive, k / n, k % n, seen[k]);
}

// the blocks of a launch: every pair of every level once
static void check_launch(const DsxTuning& t, int nlev, const int* npairs, const int* M, const int* pack) {
  int blk_end[dsx::kRowMultiMax] = {};
  const dsx::RowLaunch g = dsx::row_pack_launch(t, nlev, npairs, M, pack, blk_end);
  CHECK(g.wpb == t.row_pack_wpb && (g.wpb == 4 || g.wpb == 8), "wpb %d", g.wpb);
  CHECK(g.lds <= dsx::kLdsLimit, "lds %zu", g.lds);
  CHECK(g.grid_x == blk_end[nlev - 1], "grid %d", g.grid_x);
  std::vector<std::vector<int>> seen(nlev);
  for (int i = 0; i < nlev; ++i) {
    seen[i].assign(npairs[i], 0);
    CHECK(g.lds >= (size_t)(1 + g.wpb * pack[i]) * M[i] * dsx::kC32Bytes, "level %d: lds %zu", i, g.lds);
    CHECK(blk_end[i] > (i ? blk_end[i - 1] : 0), "blk_end[%d]", i);
  }
  for (int x = 0; x < g.grid_x; ++x) {
    int ent = 0;
    while (ent + 1 < nlev && x >= blk_end[ent]) ++ent;  // as the kernel finds its level
    const int bx = x - (ent > 0 ? blk_end[ent - 1] : 0);
    for (int wave = 0; wave < g.wpb; ++wave) {
      const int pair0 = (bx * g.wpb + wave) * pack[ent];
      const int nlive = std::max(0, std::min(pack[ent], npairs[ent] - pair0));
      // the wave's buffers end inside the block's LDS
      CHECK((size_t)M[ent] * (1 + wave * pack[ent] + pack[ent]) * dsx::kC32Bytes <= g.lds, "block %d wave %d", x, wave);
      for (int p = 0; p < nlive; ++p) ++seen[ent][pair0 + p];
    }
  }
  for (int i = 0; i < nlev; ++i)
    for (int k = 0; k < npairs[i]; ++k) CHECK(seen[i][k] == 1, "level %d pair %d covered %d times", i, k, seen[i][k]);
}

int main() {
  DsxTuning def;  // the defaults, whatever the environment says
  int Ms[6], npairs[6], pack_def[6];
  for (int li = 0; li < 6; ++li) {
    const Length& L = kLengths[li];
    const std::vector<int> rad = dsx::factorize(L.M);
    CHECK((int)rad.size() == L.npass && memcmp(rad.data(), L.radix, sizeof(int) * L.npass) == 0, "pass list of %d", L.M);
    CHECK(dsx::row_pack_reg_passes(L.npass, L.radix), "M=%d", L.M);
    int best = 1;
    double best_cost = 1e300;
    for (int P = 1; P <= dsx::kRowPackMax; ++P) {
      // the bounds, stated again: registers per pass, LDS of 16 waves on a CU
      bool regs = true;
      for (int i = 0; i < L.npass; ++i) {
        const int R = L.radix[i], rounds = (dsx::kRowPackValues + R - 1) / R;
        regs = regs && P * (L.M / R) <= 64 * rounds;
      }
      for (int wpb = 4; wpb <= 8; wpb += 4) {
        const bool lds = (size_t)(16 / wpb) * (1 + wpb * P) * L.M * 8 <= dsx::kLdsLimit;
        CHECK(dsx::row_pack_fits(L.M, L.npass, L.radix, P, wpb) == (regs && lds), "M=%d P=%d wpb=%d", L.M, P, wpb);
      }
      if (!dsx::row_pack_fits(L.M, L.npass, L.radix, P, def.row_pack_wpb)) continue;
      // the map of every pass and of the spectral step, with every count of live pairs
      for (int nlive = 1; nlive <= P; ++nlive) {
        for (int i = 0; i < L.npass; ++i) {
          const int R = L.radix[i];
          check_map(L.M, L.M / R, (dsx::kRowPackValues + R - 1) / R, P, nlive);
        }
        for (int n1 = 1; n1 <= L.M / 2 + 1; n1 += (L.M > 100 ? 7 : 1)) check_map(L.M, n1, (nlive * n1 + 63) / 64, P, nlive);
      }
      const double c = dsx::row_pack_cost(L.M, L.npass, L.radix, P);
      if (P == 1) CHECK(c >= L.cost1 - 0.5 && c <= L.cost1 + 0.5, "M=%d: cost %.1f at P = 1", L.M, c);
      if (c < best_cost) { best_cost = c; best = P; }
      // DSX_ROW_PACK = P: that factor where it fits
      DsxTuning forced;
      forced.row_pack = P;
      CHECK(dsx::row_pack_factor(forced, L.M, L.npass, L.radix) == P, "M=%d forced P=%d", L.M, P);
    }
    const int got = dsx::row_pack_factor(def, L.M, L.npass, L.radix);
    CHECK(got == best && got == L.best, "M=%d: pack factor %d, least cost at %d", L.M, got, best);
    CHECK(best_cost >= L.cost_best - 0.5 && best_cost <= L.cost_best + 0.5, "M=%d: cost %.1f at P = %d", L.M, best_cost, best);
    CHECK(dsx::row_pack_fits(L.M, L.npass, L.radix, got, def.row_pack_wpb), "M=%d P=%d", L.M, got);
    Ms[li] = L.M;
    npairs[li] = L.npairs;
    pack_def[li] = got;
  }
  // a pass list with a generic pass (prime factor 23) is not packed; the widest length of the class within the LDS bound
  {
    const int r23[2] = {23, 4};
    CHECK(dsx::row_pack_factor(def, 92, 2, r23) == 1, "generic pass");
    const std::vector<int> rad = dsx::factorize(384);
    const int P = dsx::row_pack_factor(def, 384, (int)rad.size(), rad.data());
    CHECK(P >= 1 && dsx::row_pack_fits(384, (int)rad.size(), rad.data(), P, def.row_pack_wpb), "M=384 P=%d", P);
  }
  // launches: the flagship's six levels with the default factors, then every factor, block size and pair count
  check_launch(def, 6, npairs, Ms, pack_def);
  for (int wpb = 4; wpb <= 8; wpb += 4) {
    DsxTuning t;
    t.row_pack_wpb = wpb;
    for (int P = 1; P <= dsx::kRowPackMax; ++P) {
      t.row_pack = P;
      for (int np0 = 1; np0 <= 70; ++np0) {
        int pack[6], np[6];
        for (int li = 0; li < 6; ++li) {
          pack[li] = dsx::row_pack_factor(t, Ms[li], kLengths[li].npass, kLengths[li].radix);
          CHECK(pack[li] >= 1 && pack[li] <= P, "pack %d", pack[li]);
          np[li] = std::max(1, np0 * (6 - li) / 3);
        }
        check_launch(t, 6, np, Ms, pack);
        check_launch(t, 2, np + 2, Ms + 2, pack + 2);
      }
    }
  }
  // the decision of stage_rowfilters
  {
    DsxTuning off;
    off.no_row_pack = true;
    DsxTuning forced;
    forced.row_pack_fill = 0;
    const int cus = 256;
    // a launch that fills the chip once (16 waves per CU with one pair per wave) is packed: 16 planes of 2048^2 and more
    CHECK(dsx::row_pack_runs(def, 6, 64LL * 264, cus) && dsx::row_pack_runs(def, 6, 16LL * 264, cus) && dsx::row_pack_runs(def, 2, 4096, cus),
          "row_pack_runs: full launches");
    CHECK(!dsx::row_pack_runs(def, 6, 15LL * 264, cus) && !dsx::row_pack_runs(def, 6, 264, cus) && !dsx::row_pack_runs(def, 1, 1 << 20, cus),
          "row_pack_runs: small launches, single levels");
    // the switches: never with DSX_NO_ROW_PACK, whatever the size with DSX_ROW_PACK_FILL = 0
    CHECK(!dsx::row_pack_runs(off, 6, 64LL * 264, cus) && dsx::row_pack_runs(forced, 2, 8, cus) && !dsx::row_pack_runs(forced, 1, 8, cus),
          "row_pack_runs: switches");
    forced.no_row_pack = true;
    CHECK(!dsx::row_pack_runs(forced, 6, 64LL * 264, cus), "row_pack_runs: DSX_NO_ROW_PACK wins");
  }
  printf("{\"ok\": %s, \"checked\": %lld, \"failed\": %d, \"pack\": [%d, %d, %d, %d, %d, %d]}\n", g_failed ? "false" : "true",
         g_checked, g_failed, pack_def[0], pack_def[1], pack_def[2], pack_def[3], pack_def[4], pack_def[5]);
  return g_failed ? 1 : 0;
}
