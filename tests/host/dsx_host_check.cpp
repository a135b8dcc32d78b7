// Host-side (g++) checks of the code the HIP kernels share with the CPU:
//   fft  <M>                     Stockham passes built from dsx_fft_core.h vs a naive DFT
//   rows <H> <W> <sigma> <level> <lvl>  emulates k_rowfilter's spectral pipeline for one level with the
//                                planned (M, K, radices, G tables) and compares with the exact
//                                length-w circular operator of the reference (packed-index gains)
//   plan <H> <W> <s0> <l0> <s1> <l1>    prints the plan (levels, dims, M, K, radices)
//   chain key=value ...          the launches dsx_chain.h decides for one run call (switches: the DSX_* environment)
//   chain-rules                  sweeps the geometry rules the kernels rely on (tests/test_chain_host.py)
//   genlds                       dynamic LDS of k_fwd_gen / k_inv_gen per tap count (tests/test_wavelet_gen_cases_host.py)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <complex>
#include <vector>

#include "../../aind_smartspim_destripe_amd/csrc/dsx_fft_core.h"
#include "../../aind_smartspim_destripe_amd/csrc/dsx_plan.h"
#include "../../aind_smartspim_destripe_amd/csrc/dsx_chain.h"

typedef std::complex<double> cd;

static void run_passes(std::vector<dsx_c32>& buf, const std::vector<dsx_c32>& tw, const int* radix, int npass) {
  const int M = (int)buf.size();
  int s = 1;
  for (int pi = 0; pi < npass; ++pi) {
    const int R = radix[pi];
    const float inv_s = 1.0f / (float)s;
    const int nb = M / R;
    if (R <= 20 || R == 25) {
      // read phase for every butterfly, then compute + scatter phase (what a wave does)
      std::vector<dsx_c32> regs((size_t)nb * R);
      for (int b = 0; b < nb; ++b) {
        switch (R) {
          case 2: dsx_bfly_load<2>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 3: dsx_bfly_load<3>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 4: dsx_bfly_load<4>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 5: dsx_bfly_load<5>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 7: dsx_bfly_load<7>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 11: dsx_bfly_load<11>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 13: dsx_bfly_load<13>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 17: dsx_bfly_load<17>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 19: dsx_bfly_load<19>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 6: dsx_bfly_load<6>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 8: dsx_bfly_load<8>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 9: dsx_bfly_load<9>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 10: dsx_bfly_load<10>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 12: dsx_bfly_load<12>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 15: dsx_bfly_load<15>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 16: dsx_bfly_load<16>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 20: dsx_bfly_load<20>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
          case 25: dsx_bfly_load<25>(buf.data(), b, nb, &regs[(size_t)b * R]); break;
        }
      }
      for (int b = 0; b < nb; ++b) {
        switch (R) {
          case 2: dsx_bfly_store<2>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 3: dsx_bfly_store<3>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 4: dsx_bfly_store<4>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 5: dsx_bfly_store<5>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 7: dsx_bfly_store<7>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 11: dsx_bfly_store<11>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 13: dsx_bfly_store<13>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 17: dsx_bfly_store<17>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 19: dsx_bfly_store<19>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R]); break;
          case 6: dsx_bfly_store<6>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 8: dsx_bfly_store<8>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 9: dsx_bfly_store<9>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 10: dsx_bfly_store<10>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 12: dsx_bfly_store<12>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 15: dsx_bfly_store<15>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 16: dsx_bfly_store<16>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 20: dsx_bfly_store<20>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
          case 25: dsx_bfly_store<25>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], s * R == M); break;
        }
      }
    } else {
      std::vector<dsx_c32> acc(M);
      for (int o = 0; o < M; ++o) acc[o] = dsx_generic_output(buf.data(), tw.data(), o, M, s, inv_s, R);
      buf = acc;
    }
    s *= R;
  }
}

static std::vector<dsx_c32> twiddles(int M);

// The forward plan of the level-1 row filter at 2048 columns (StaticFft<1>::run_forward in csrc/dsx_kernels.h): passes
// 6, 9 in full, then the radix-19 pass with only the output pairs k <= KO -- every bin |k| <= kcut must be the DFT.
template <int KO>
static double pruned_1026(int kcut) {
  const int M = 1026;
  std::vector<dsx_c32> buf(M), tw = twiddles(M);
  std::vector<cd> x(M);
  srand(1026 + KO);
  for (int i = 0; i < M; ++i) {
    x[i] = cd(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
    buf[i] = dsx_mk((float)x[i].real(), (float)x[i].imag());
  }
  const int first[2] = {6, 9};
  // (run_passes derives the sub-transform stride from the radices it is given: 1, then 6)
  {
    int s = 1;
    for (int pi = 0; pi < 2; ++pi) {
      const int R = first[pi], nb = M / R;
      const float inv_s = 1.0f / (float)s;
      std::vector<dsx_c32> regs((size_t)nb * R);
      for (int b = 0; b < nb; ++b) {
        if (R == 6) dsx_bfly_load<6>(buf.data(), b, nb, &regs[(size_t)b * R]);
        else dsx_bfly_load<9>(buf.data(), b, nb, &regs[(size_t)b * R]);
      }
      for (int b = 0; b < nb; ++b) {
        if (R == 6) dsx_bfly_store<6>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], false);
        else dsx_bfly_store<9>(buf.data(), tw.data(), b, s, inv_s, &regs[(size_t)b * R], false);
      }
      s *= R;
    }
  }
  {
    const int R = 19, nb = M / R, s = 54;
    std::vector<dsx_c32> regs((size_t)nb * R);
    for (int b = 0; b < nb; ++b) dsx_bfly_load<19>(buf.data(), b, nb, &regs[(size_t)b * R]);
    for (int b = 0; b < nb; ++b) dsx_bfly_store<19, 9, KO>(buf.data(), tw.data(), b, s, 1.0f / 54.0f, &regs[(size_t)b * R], true);
  }
  double err = 0, nrm = 0;
  for (int k = 0; k < M; ++k) {
    if (k > kcut && k < M - kcut) continue;
    cd acc = 0;
    for (int j = 0; j < M; ++j) acc += x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % M) / M);
    err = fmax(err, std::abs(acc - cd(buf[k].x, buf[k].y)));
    nrm = fmax(nrm, std::abs(acc));
  }
  return err / nrm;
}

// The power-of-two plans with bank-swizzled addressing (dsx_idx_swz on the row buffer AND the twiddle table, as
// StaticFft<3> / <5> run them): the data is placed at sw(i), the twiddles at sw(t), every pass addresses through the
// policy, and the result is read back from sw(k) -- it must be the DFT exactly as without the swizzle.
template <int R>
static void swz_pass(std::vector<dsx_c32>& buf, const std::vector<dsx_c32>& tw, int M, int s) {
  const int nb = M / R;
  std::vector<dsx_c32> regs((size_t)nb * R);
  for (int b = 0; b < nb; ++b) dsx_bfly_load<R, (R - 1) / 2, dsx_idx_swz>(buf.data(), b, nb, &regs[(size_t)b * R]);
  for (int b = 0; b < nb; ++b)
    dsx_bfly_store<R, (R - 1) / 2, (R - 1) / 2, dsx_idx_swz>(buf.data(), tw.data(), b, s, 1.0f / (float)s, &regs[(size_t)b * R], s * R == M);
}

// the same passes with the addressing written out (dsx_swz_load / dsx_swz_store): must give the very same bits
template <int R, int M, int S>
static void swz_pass_fast(std::vector<dsx_c32>& buf, const std::vector<dsx_c32>& tw) {
  const int nb = M / R;
  std::vector<dsx_c32> regs((size_t)nb * R);
  for (int b = 0; b < nb; ++b) dsx_swz_load<R, M>(buf.data(), b, &regs[(size_t)b * R]);
  for (int b = 0; b < nb; ++b) dsx_swz_store<R, M, S>(buf.data(), tw.data(), b, &regs[(size_t)b * R]);
}

static double swizzled(int M) {
  std::vector<dsx_c32> buf(M), plain = twiddles(M), tw(M);
  std::vector<cd> x(M);
  srand(M + 7);
  for (int i = 0; i < M; ++i) {
    x[i] = cd(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
    buf[dsx_idx_swz::at(i)] = dsx_mk((float)x[i].real(), (float)x[i].imag());
    tw[dsx_idx_swz::at(i)] = plain[i];
  }
  std::vector<dsx_c32> fast = buf;
  if (M == 2048) { swz_pass<16>(buf, tw, M, 1); swz_pass<16>(buf, tw, M, 16); swz_pass<8>(buf, tw, M, 256); }
  else { swz_pass<16>(buf, tw, M, 1); swz_pass<8>(buf, tw, M, 16); swz_pass<8>(buf, tw, M, 128); }
  if (M == 2048) { swz_pass_fast<16, 2048, 1>(fast, tw); swz_pass_fast<16, 2048, 16>(fast, tw); swz_pass_fast<8, 2048, 256>(fast, tw); }
  else { swz_pass_fast<16, 1024, 1>(fast, tw); swz_pass_fast<8, 1024, 16>(fast, tw); swz_pass_fast<8, 1024, 128>(fast, tw); }
  for (int i = 0; i < M; ++i)
    if (memcmp(&fast[i], &buf[i], sizeof(dsx_c32)) != 0) return 1.0;  // written-out addressing differs from the policy
  double err = 0, nrm = 0;
  for (int k = 0; k < M; ++k) {
    cd acc = 0;
    for (int j = 0; j < M; ++j) acc += x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % M) / M);
    const dsx_c32 y = buf[dsx_idx_swz::at(k)];
    err = fmax(err, std::abs(acc - cd(y.x, y.y)));
    nrm = fmax(nrm, std::abs(acc));
  }
  return err / nrm;
}

static int cmd_swz() {
  printf("{\"m2048\": %.3e, \"m1024\": %.3e}\n", swizzled(2048), swizzled(1024));
  return 0;
}

static int cmd_pruned() {
  // kcut of the production configs at 2048 columns: 103 (cells) / 206 (no cells); 107 / 215 are the last bins 2 / 4 pairs reach
  printf("{\"ko2_kcut103\": %.3e, \"ko2_kcut107\": %.3e, \"ko4_kcut206\": %.3e, \"ko4_kcut215\": %.3e, \"ko9_full\": %.3e}\n",
         pruned_1026<2>(103), pruned_1026<2>(107), pruned_1026<4>(206), pruned_1026<4>(215), pruned_1026<9>(512));
  return 0;
}

static std::vector<dsx_c32> twiddles(int M) {
  std::vector<dsx_c32> tw(M);
  for (int t = 0; t < M; ++t) {
    const double a = -2.0 * M_PI * t / M;
    tw[t] = dsx_mk((float)cos(a), (float)sin(a));
  }
  return tw;
}

static int cmd_fft(int M) {
  std::vector<int> rad = dsx::factorize(M);
  std::vector<dsx_c32> buf(M);
  std::vector<cd> x(M);
  srand(M);
  for (int i = 0; i < M; ++i) {
    x[i] = cd(rand() / (double)RAND_MAX - 0.5, rand() / (double)RAND_MAX - 0.5);
    buf[i] = dsx_mk((float)x[i].real(), (float)x[i].imag());
  }
  run_passes(buf, twiddles(M), rad.data(), (int)rad.size());
  double err = 0, nrm = 0;
  for (int k = 0; k < M; ++k) {
    cd acc = 0;
    for (int j = 0; j < M; ++j) acc += x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % M) / M);
    err = fmax(err, std::abs(acc - cd(buf[k].x, buf[k].y)));
    nrm = fmax(nrm, std::abs(acc));
  }
  printf("{\"M\": %d, \"npass\": %d, \"rel_err\": %.3e}\n", M, (int)rad.size(), err / nrm);
  return 0;
}

static int cmd_plan(int H, int W, double s0, int l0, double s1, int l1, dsx::Plan& p, bool print) {
  dsx::HostCfg cfg[2] = {{l0, s0, 12.0}, {l1, s1, 3.0}};
  std::string e = dsx::build_plan(H, W, cfg, p);
  if (!e.empty()) {
    printf("{\"error\": \"%s\"}\n", e.c_str());
    return 1;
  }
  if (!print) return 0;
  printf("{\"H\": %d, \"W\": %d, \"Hout\": %d, \"Wout\": %d, \"L\": %d, \"plane_floats\": %lld, \"levels\": [", p.H, p.W,
         p.Hout, p.Wout, p.L, p.plane_floats);
  for (int l = 0; l < p.L; ++l) {
    const dsx::LevelPlan& lp = p.lv[l];
    printf("%s{\"h\": %d, \"w\": %d, \"ld\": %d, \"M\": %d, \"K\": %d, \"radix\": [", l ? ", " : "", lp.h, lp.w, lp.ld, lp.M,
           lp.K);
    for (int i = 0; i < lp.npass; ++i) printf("%s%d", i ? ", " : "", lp.radix[i]);
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

// Emulate the spectral pipeline of k_rowfilter for two random rows at one level and compare with the
// exact operator  LP(x) = irfft_packed(rfft_packed(x) * e),  e[j] = exp(-j^2 / (2 s^2)).
static int cmd_rows(int H, int W, double sigma, int level, int lvl) {
  dsx::Plan p;
  if (cmd_plan(H, W, sigma, level, sigma, level, p, false)) return 1;
  if (lvl >= p.L) { printf("{\"error\": \"level out of range\"}\n"); return 1; }
  const dsx::LevelPlan& lp = p.lv[lvl];
  const int N = lp.w, M = lp.M, K = lp.K;
  const double s = lp.h * (sigma / (double)std::min(H, W));
  std::vector<double> xa(N), xb(N);
  srand(N * 7 + lvl);
  for (int n = 0; n < N; ++n) {
    xa[n] = rand() / (double)RAND_MAX - 0.3;
    xb[n] = rand() / (double)RAND_MAX - 0.6;
  }
  // exact reference operator in double: Y[k] = ep X[k] + em X[N-k]
  std::vector<double> ep, em;
  dsx::packed_gains(N, s, ep, em);
  auto exact = [&](const std::vector<double>& x) {
    std::vector<cd> X(N), Y(N);
    for (int k = 0; k < N; ++k) {
      cd acc = 0;
      for (int j = 0; j < N; ++j) acc += x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % N) / N);
      X[k] = acc;
    }
    for (int k = 0; k < N; ++k) Y[k] = ep[k] * X[k] + em[k] * X[(N - k) % N];
    std::vector<double> y(N);
    for (int n = 0; n < N; ++n) {
      cd acc = 0;
      for (int k = 0; k < N; ++k) acc += Y[k] * std::polar(1.0, 2.0 * M_PI * (double)((long long)n * k % N) / N);
      y[n] = acc.real() / N;
    }
    return y;
  };
  std::vector<double> ya = exact(xa), yb = exact(xb);
  // kernel pipeline in float
  std::vector<dsx_c32> buf(M, dsx_mk(0.f, 0.f));
  for (int n = 0; n < N; ++n) {
    dsx_c32 z = dsx_mk((float)xa[n], (float)xb[n]);
    buf[K + n] = z;
    if (K > 0) {
      if (n <= K) buf[K + N + n] = z;
      if (n >= N - K) buf[n - (N - K)] = z;
    }
  }
  std::vector<dsx_c32> tw(M);
  for (int t = 0; t < M; ++t) tw[t] = dsx_mk(p.consts[lp.tw_off + t].re, p.consts[lp.tw_off + t].im);
  run_passes(buf, tw, lp.radix, lp.npass);
  const dsx::C32* g1 = &p.consts[lp.g_off[1]];
  const dsx::C32* g2 = g1 + M;
  std::vector<dsx_c32> v(M);
  for (int k = 0; k < M; ++k) {
    dsx_c32 u = buf[k], ur = buf[k == 0 ? 0 : M - k];
    dsx_c32 r = dsx_add(dsx_mul(dsx_mk(g1[k].re, g1[k].im), u), dsx_mul(dsx_mk(g2[k].re, g2[k].im), ur));
    v[k] = dsx_mk(r.y, r.x);
  }
  run_passes(v, tw, lp.radix, lp.npass);
  double err = 0, nrm = 0;
  for (int n = 0; n < N; ++n) {
    const double la = v[K + n].y / M, lb = v[K + n].x / M;
    err = fmax(err, fmax(fabs(la - ya[n]), fabs(lb - yb[n])));
    nrm = fmax(nrm, fmax(fabs(ya[n]), fabs(yb[n])));
  }
  printf("{\"N\": %d, \"M\": %d, \"K\": %d, \"rel_err\": %.3e}\n", N, M, K, err / nrm);
  return 0;
}


// ---- chain: the launches of one dsx_run_device call, in enqueue order, spelled as a kernel trace spells them ----------
struct ChainOut {
  bool first = true;
  // M: transform length of a row-filter launch (the longest of a merged one), 0 elsewhere
  void put(const char* name, int gx, int gy, int gz, int block, size_t lds, int M = 0) {
    printf("%s[\"%s\", [%d, %d, %d], %d, %zu, %d]", first ? "" : ",\n ", name, gx, gy, gz, block, lds, M);
    first = false;
  }
};

static void chain_hist(ChainOut& o, const dsx::Plan& p, const DsxTuning& t, const dsx::ChainShape& sh, int nb, int l0, int l1) {
  int blocks = 0;
  for (int l = l0; l < l1; ++l) {
    const int rows = dsx::hist_rows_per_block(t, p.lv[l].h, p.lv[l].w, nb);
    blocks += (p.lv[l].h + rows - 1) / rows;
  }
  if (sh.thresholds && l1 > l0) o.put("k_hist", blocks, nb, 1, 64 * dsx::kHistWaves, 0);
}

static void chain_row(ChainOut& o, const DsxTuning& t, const dsx::LevelPlan& lp, int nb) {
  const dsx::RowClass c = dsx::classify_row(lp);
  const int npairs = (lp.h + 1) / 2;
  if (c.wide) return o.put("k_rowfilter_wide", npairs, nb, 1, dsx::kWideThreads, (size_t)lp.M * dsx::kC32Bytes, lp.M);
  char name[96];
  snprintf(name, sizeof(name), "k_rowfilter<%d, %d, %d, %d, %d>", c.cpl, c.gf, c.nt, c.halo, c.plan);
  const dsx::RowLaunch g = dsx::rowfilter_launch(t, c.cpl, lp.M, npairs);
  o.put(name, g.grid_x, nb, 1, 64 * g.wpb, g.lds, lp.M);
}

// one cohort part (run_cohort of csrc/dsx.hip, stage by stage)
static void chain_part(ChainOut& o, const dsx::Plan& p, const DsxTuning& t, const dsx::ChainCall& call, int cus, int flen,
                       size_t minmax_addr) {
  const dsx::ChainShape sh = dsx::chain_shape(p, t, call);
  const int L = p.L, nb = call.nb, kind0 = call.in_u16 ? 0 : 1;
  char name[96];
  const dsx::ZeroLaunch z = dsx::zero_launch(nb, std::max(1, L), minmax_addr);
  if (z.grid_x > 0) o.put("k_zero3", z.grid_x, 1, 1, 256, 0);
  for (int l = 0; l < L; ++l) {  // forward
    if (sh.fuse12 && l == 1) continue;
    if (sh.generic) {
      snprintf(name, sizeof(name), "k_fwd_gen<%d>", l > 0 ? 2 : kind0);
      o.put(name, (p.lv[l].w + dsx::kGenTW - 1) / dsx::kGenTW, (p.lv[l].h + dsx::kGenTH - 1) / dsx::kGenTH, nb, 256,
            dsx::gen_fwd_lds_bytes(flen));
      continue;
    }
    const dsx::MarchLaunch m = dsx::fwd_launch(p, sh, t, cus, nb, call.alone, l);
    const bool fused = sh.fuse12 && l == 0;
    snprintf(name, sizeof(name), "k_fwd_march<%d, %s, %d>", l > 0 ? 2 : kind0, fused ? "true" : "false", m.wpb);
    o.put(name, m.grid_x, nb, 1, 64 * m.wpb, 0);
    if (sh.split && l == 0) chain_hist(o, p, t, sh, nb, 0, 2);
  }
  chain_hist(o, p, t, sh, nb, sh.split ? 2 : 0, L);  // thresholds
  if (L > 0 && sh.thresholds) o.put("k_otsu", L, nb, 1, 64, 0);
  if (call.stop_after == 1) return;
  int multi_pairs[dsx::kRowMultiMax], multi_m[dsx::kRowMultiMax], multi_lv[dsx::kRowMultiMax], nmulti = 0;
  for (int l = 0; l < L; ++l) {  // row filters
    if (sh.rf_plan != 0 && l == 0) continue;
    const bool own_stream = !(sh.split_inv && l < 2);
    if (dsx::row_multi_takes(sh, own_stream, p.lv[l].M, nmulti)) {
      multi_pairs[nmulti] = (p.lv[l].h + 1) / 2;
      multi_m[nmulti] = p.lv[l].M;
      multi_lv[nmulti++] = l;
      continue;
    }
    chain_row(o, t, p.lv[l], nb);
  }
  if (nmulti == 1) chain_row(o, t, p.lv[multi_lv[0]], nb);
  if (nmulti > 1) {
    int blk_end[dsx::kRowMultiMax];
    const dsx::RowLaunch g = dsx::row_multi_launch(nmulti, multi_pairs, multi_m, blk_end);
    o.put("k_rowfilter_multi<6>", g.grid_x, nb, 1, 64 * g.wpb, g.lds, *std::max_element(multi_m, multi_m + nmulti));
  }
  if (call.stop_after == 2) return;
  for (int l = L - 1; l >= (L > 0 ? 0 : -1); --l) {  // inverse + finish
    if (sh.fuse21 && l == 1) continue;
    const bool last = l <= 0;
    const int hout = last ? p.Hout : p.lv[l - 1].h, wout = last ? p.Wout : p.lv[l - 1].w;
    if (sh.generic) {
      snprintf(name, sizeof(name), "k_inv_gen<%d>", last ? kind0 : 2);
      o.put(name, (wout + dsx::kGenOW - 1) / dsx::kGenOW, (hout + dsx::kGenOH - 1) / dsx::kGenOH, nb, 256,
            dsx::gen_inv_lds_bytes(flen));
      continue;
    }
    const bool fused = sh.fuse21 && last;
    if (fused && sh.rf_plan != 0) {
      const dsx::RowClass c = dsx::classify_row(p.lv[0]);
      const dsx::RowLaunch g = dsx::rowfinal_launch(p.lv[0].M, hout);
      snprintf(name, sizeof(name), "k_rowfinal<%d, %d, %d, %d, %d>", c.cpl, c.gf, c.nt, c.halo, sh.rf_plan);
      o.put(name, g.grid_x, nb, 1, 64 * g.wpb, g.lds, p.lv[0].M);
      continue;
    }
    const dsx::MarchLaunch m = dsx::inv_launch(sh, t, cus, nb, l, hout, wout);
    snprintf(name, sizeof(name), "k_inv_march<%d, %s, %d>", last ? kind0 : 2, fused ? "true" : "false", m.wpb);
    o.put(name, m.grid_x, nb, 1, 64 * m.wpb, 0);
  }
}

static int cmd_chain(int argc, char** argv) {
  auto arg = [&](const char* key, double fallback) {
    const size_t n = strlen(key);
    for (int i = 2; i < argc; ++i)
      if (!strncmp(argv[i], key, n) && argv[i][n] == '=') return atof(argv[i] + n + 1);
    return fallback;
  };
  const int H = (int)arg("H", 0), W = (int)arg("W", 0), n = (int)arg("n", 1), max_batch = (int)arg("max_batch", n);
  const int flen = (int)arg("flen", 0);  // taps of a filter bank (dsx_set_wavelet); 0: db3
  const int streams = (int)arg("streams", 4), cus = (int)arg("cus", 256), calls = (int)arg("calls", 1);
  const bool in_u16 = arg("in_u16", 1) != 0, out_u16 = arg("out_u16", 1) != 0, stack = arg("stack", 0) != 0;
  const size_t in_off = (size_t)arg("in_off", 0), out_off = (size_t)arg("out_off", 0);
  dsx::HostCfg cfg[2] = {{(int)arg("l0", -1), arg("s0", 64.0), 3.0}, {(int)arg("l1", -1), arg("s1", 128.0), 12.0}};
  dsx::Plan p;
  const std::string e = dsx::build_plan(H, W, cfg, p, flen ? flen : dsx::kFilterLen);
  if (!e.empty()) {
    printf("{\"error\": \"%s\"}\n", e.c_str());
    return 1;
  }
  DsxTuning t;
  dsx::read_tuning(t);
  const int Lc = std::max(1, p.L);
  const size_t in_plane = (size_t)p.H * p.W * (in_u16 ? 2 : 4), out_plane = (size_t)p.Hout * p.Wout * (out_u16 ? 2 : 4);
  ChainOut o;
  printf("[");
  for (int call_i = 0; call_i < calls; ++call_i)
    for (int start = 0; start < n; start += max_batch) {
      const int nb = std::min(max_batch, n - start);
      const int parts = dsx::cohort_parts(streams, nb, stack), per = (nb + parts - 1) / parts;
      for (int i = 0; i < parts; ++i) {
        const int po = i * per;
        if (nb - po <= 0) break;
        dsx::ChainCall c;
        c.in_u16 = in_u16; c.out_u16 = out_u16;
        c.nb = std::min(per, nb - po);
        c.aligned16 = (((in_off + (start + po) * in_plane) | (out_off + (start + po) * out_plane)) & 15) == 0;
        c.bank = flen > 0;
        c.stop_after = (int)arg("stop_after", 0);
        c.st_march = arg("st_march", 0) != 0;
        c.alone = parts <= 1;
        c.has_helper = dsx::part_uses_helper(t, c.alone, c.stop_after != 0);
        // the control block is one allocation: stats of max_batch planes, then minmax (2 Lc words per plane)
        chain_part(o, p, t, c, cus, flen, dsx::kPlaneStatsBytes * max_batch + sizeof(unsigned) * 2 * Lc * (size_t)po);
      }
    }
  printf("]\n");
  return 0;
}

// ---- chain-rules: what the kernels rely on, over the value lists of tools/fuzz_parity.py's switch table ---------------
#define RULE(cond, ...)                                          \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("{\"ok\": false, \"rule\": \"%s\", \"at\": \"", #cond); \
      printf(__VA_ARGS__);                                       \
      printf("\"}\n");                                           \
      return 1;                                                  \
    }                                                            \
  } while (0)

static int cmd_chain_rules() {
  long long checked = 0;
  const int nbs[] = {1, 2, 15, 16, 64, 256}, rows_l[] = {1, 2, 3, 9, 24, 25, 130, 1026}, wpbs[] = {0, 8}, cus_l[] = {64, 256, 304};
  const int seg_min[] = {4, 2, 3, 5, 8, 24}, waves[] = {4096, 64, 256, 1024, 16384}, hist_rows[] = {0, 1, 32, 128, 256};
  const int row_wpb[] = {0, 4, 5, 6, 7, 8};
  DsxTuning t;
  for (int sm : seg_min) for (int mw : waves) for (int nq = 0; nq < 2; ++nq) {
    t.seg_min_rows = sm; t.march_waves = mw; t.no_quant = nq != 0;
    for (int nb : nbs) for (int rows : rows_l) for (int wpb : wpbs) for (int cus : cus_l)
      for (int nstrips : {1, 9, 17, 34}) for (int coarse = 0; coarse < 2; ++coarse) {
        const dsx::MarchSeg g = dsx::march_segments(t, cus, nb, nstrips, rows, wpb, wpb ? 2 : 0, coarse != 0);
        RULE(g.nseg >= 1 && g.rows_per_seg >= 1 && g.rows_per_seg <= 4096 && (long long)g.nseg * g.rows_per_seg >= rows &&
                 (long long)(g.nseg - 1) * g.rows_per_seg < rows,
             "nb %d rows %d wpb %d cus %d nstrips %d coarse %d seg_min %d waves %d: nseg %d rps %d", nb, rows, wpb, cus, nstrips,
             coarse, sm, mw, g.nseg, g.rows_per_seg);
        // the fused final kernel: segments start at even level-1 rows, and still cover hout = 2 rows - 1 and 2 rows
        dsx::ChainShape sh = {};
        sh.fuse21 = true;
        for (int hout : {2 * rows - 1, 2 * rows}) {
          const dsx::MarchLaunch m = dsx::inv_launch(sh, t, cus, nb, 0, hout, 256 * nstrips);
          RULE((m.rows_per_seg & 1) == 0 && (long long)m.nseg * m.rows_per_seg >= rows &&
                   (long long)(m.nseg - 1) * m.rows_per_seg < rows && m.nseg >= 1,
               "fused final: nb %d hout %d cus %d seg_min %d waves %d: nseg %d rps %d", nb, hout, cus, sm, mw, m.nseg, m.rows_per_seg);
        }
        ++checked;
      }
  }
  for (int hr : hist_rows) for (int nb : nbs) for (int h : rows_l) for (int w = 1; w <= 18432; ++w) {
    t.hist_rows = hr;
    const int r = dsx::hist_rows_per_block(t, h, w, nb);
    RULE(r >= 1 && r * (4 * (w >> 8) + 4) <= 65535, "hist_rows %d nb %d h %d w %d: %d rows", hr, nb, h, w, r);
    ++checked;
  }
  for (int rw : row_wpb) for (int M = 1; M <= 2304; ++M) {
    t.row_wpb = rw;
    const dsx::RowLaunch g = dsx::rowfilter_launch(t, dsx::cpl_class(M), M, 1000);
    RULE(g.lds <= dsx::kLdsLimit && g.wpb >= 4 && g.wpb <= dsx::kRowMaxWaves && (long long)g.grid_x * g.wpb >= 1000,
         "row_wpb %d M %d: wpb %d lds %zu", rw, M, g.wpb, g.lds);
    ++checked;
  }
  // a non-zero k_rowfinal plan id is the id the classifier gives level 1; blk_end of the merged coarse launch
  std::vector<int> widths = {2048, 2000, 1800, 1024, 4800};  // the compile-time plans, and a wide one
  for (int W = 64; W <= 2304; W += 56) widths.push_back(W);
  for (int W : widths) {
    dsx::HostCfg cfg[2] = {{-1, 64.0, 3.0}, {-1, 128.0, 12.0}};
    dsx::Plan p;
    if (!dsx::build_plan(64, W, cfg, p).empty()) continue;
    for (int wide = 0; wide < 2; ++wide) {
      const int id = dsx::rowfinal_plan(p, true, true, true, wide != 0);
      RULE(id == 0 || id == dsx::classify_row(p.lv[0]).plan, "W %d wide %d: rowfinal plan %d", W, wide, id);
    }
    int np[dsx::kRowMultiMax], M[dsx::kRowMultiMax], blk_end[dsx::kRowMultiMax], nl = 0;
    for (int l = 0; l < p.L && nl < dsx::kRowMultiMax; ++l)
      if (p.lv[l].M <= 384) { np[nl] = (p.lv[l].h + 1) / 2; M[nl++] = p.lv[l].M; }
    const dsx::RowLaunch g = dsx::row_multi_launch(nl, np, M, blk_end);
    for (int i = 0; i < nl; ++i) RULE(blk_end[i] > (i ? blk_end[i - 1] : 0), "W %d: blk_end[%d] = %d", W, i, blk_end[i]);
    RULE(nl == 0 || blk_end[nl - 1] == g.grid_x, "W %d: grid %d", W, g.grid_x);
    RULE(g.lds <= dsx::kLdsLimit, "W %d: merged launch lds %zu", W, g.lds);
    ++checked;
  }
  // the table of compile-time plans agrees with itself: the radices make M, cpl is M's class, and the classifier gives
  // a row of exactly these numbers the row's id (every width of the slot structure gf / nt)
  for (int id = 1; id <= dsx::kRowPlanCount; ++id) {
    const dsx::RowPlan& rp = dsx::row_plan(id);
    RULE(rp.radix[0] * rp.radix[1] * rp.radix[2] == rp.M, "plan %d: radices of M %d", id, rp.M);
    RULE(dsx::cpl_class(rp.M) == rp.cpl, "plan %d: cpl %d", id, rp.cpl);
    for (int w = 256 * rp.gf + 64 * (rp.nt - 1) + 1; w <= 256 * rp.gf + 64 * rp.nt && w < 256 * (rp.gf + 1) && w <= rp.M; ++w) {
      const dsx::RowClass c = dsx::classify_row(rp.M, w, /*K=*/rp.halo, 3, rp.radix);
      RULE(!c.wide && c.plan == id && c.cpl == rp.cpl && c.gf == rp.gf && c.nt == rp.nt && c.halo == rp.halo,
           "plan %d w %d: classified as <%d, %d, %d, %d, %d>", id, w, c.cpl, c.gf, c.nt, c.halo, c.plan);
      ++checked;
    }
  }
  printf("{\"ok\": true, \"checked\": %lld}\n", checked);
  return 0;
}

// genlds: the dynamic LDS k_fwd_gen / k_inv_gen are launched with, per even tap count up to kMaxTaps' 104
static int cmd_genlds() {
  printf("{\"limit\": %zu, \"taps\": {", dsx::kLdsLimit);
  for (int F = 2; F <= 104; F += 2)
    printf("%s\"%d\": [%zu, %zu]", F > 2 ? ", " : "", F, dsx::gen_fwd_lds_bytes(F), dsx::gen_inv_lds_bytes(F));
  printf("}}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "genlds")) return cmd_genlds();
  if (argc >= 2 && !strcmp(argv[1], "chain")) return cmd_chain(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "chain-rules")) return cmd_chain_rules();
  if (argc >= 3 && !strcmp(argv[1], "fft")) return cmd_fft(atoi(argv[2]));
  if (argc >= 8 && !strcmp(argv[1], "plan")) {
    dsx::Plan p;
    return cmd_plan(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atoi(argv[5]), atof(argv[6]), atoi(argv[7]), p, true);
  }
  if (argc >= 7 && !strcmp(argv[1], "rows"))
    return cmd_rows(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atoi(argv[5]), atoi(argv[6]));
  if (argc >= 2 && !strcmp(argv[1], "pruned")) return cmd_pruned();
  if (argc >= 2 && !strcmp(argv[1], "swz")) return cmd_swz();
  fprintf(stderr, "usage: pruned | swz | fft M | plan H W s0 l0 s1 l1 | rows H W sigma level lvl | chain key=value ... | chain-rules | genlds\n");
  return 2;
}
