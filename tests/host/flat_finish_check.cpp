// Host build of the native finish of a flat (csrc/dsx_smooth.h: what dsx_gauss_smooth_f64_ref and dsx_flat_finish_ref
// run), for tests/test_flat_finish_host.py:
//   flat_finish_check smooth <plane.raw> <H> <W> <taps.raw> <radius> <in_place> <result.out>
//       reads H * W float64 and radius + 1 float64 taps, writes the smoothed plane; in_place != 0 smooths into the input
//   flat_finish_check finish <rank.raw> <valid.raw> <Hs> <Ws> <H> <W> <n_q> <taps.raw> <radius> <floor> <result.out>
//       reads n_q * Hs * Ws and Hs * Ws uint16, writes flat [H * W] float32 followed by dark when n_q == 2; exit code 6
//       when no pixel of the image is seen
// Planes, taps and results live in heap buffers of exactly their own size, so a sanitizer build sees a read or a write
// outside them.  Both modes first walk the launch geometry of the plane over every radius: the tiles cover the plane
// exactly, the windows fit the LDS the launch may ask for, two column-pass blocks fit a CU's 160 KiB at r = 128, and
// every window index the kernels form lies inside the window.
#include "../../aind_smartspim_destripe_amd/csrc/dsx_smooth.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sm = dsx::sm;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
  fclose(f);
  return ok;
}

template <class T>
static bool write_some(FILE* f, const std::vector<T>& v) {
  if (v.empty()) return true;
  return fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

static bool geometry_holds(long long H, long long W) {
  for (int r = 0; r <= sm::kSmMaxRadius; ++r) {
    const sm::Geometry g = sm::geometry(H, W, r);
    if (g.col_tx * (sm::kSmThreads / g.col_tx) * 4 != g.col_tx * g.col_ty) return false;  // four rows per thread
    if (g.row_tx * (sm::kSmThreads / g.row_tx) * 4 != g.row_tx * g.row_ty) return false;
    if ((long long)g.col_bx * g.col_tx < W || (long long)(g.col_bx - 1) * g.col_tx >= W) return false;
    if ((long long)g.col_by * g.col_ty < H || (long long)(g.col_by - 1) * g.col_ty >= H) return false;
    if ((long long)g.row_bx * g.row_tx < W || (long long)(g.row_bx - 1) * g.row_tx >= W) return false;
    if ((long long)g.row_by * g.row_ty < H || (long long)(g.row_by - 1) * g.row_ty >= H) return false;
    if (g.col_lds > sm::kSmMaxLds || g.row_lds > sm::kSmMaxLds || sm::kSmMaxLds > 160 * 1024) return false;
    if (r <= 128 && (2 * g.col_lds > 160 * 1024 || 2 * g.row_lds > 160 * 1024)) return false;
    if (g.row_pad < r || (g.row_pad & 1) || (g.row_pitch & 1)) return false;
    // the lowest and the highest window index of a tap: centre - r and centre + r of the first and the last output
    if (g.col_rows != g.col_ty + 2 * r || (g.col_ty - 1 + r) + r >= g.col_rows) return false;
    if (g.row_pad - r < 0 || g.row_pad + (g.row_tx - 1) + r >= g.row_pitch) return false;
    if ((unsigned long long)g.col_bx * g.col_by > 0x7fffffffull || (unsigned long long)g.row_bx * g.row_by > 0x7fffffffull) return false;
  }
  for (long long n = 1; n <= 5; ++n)  // the fold against np.pad(mode="symmetric") written out
    for (long long j = -40; j <= 40; ++j) {
      long long q = j;
      while (q < 0 || q >= n) q = q < 0 ? -q - 1 : 2 * n - 1 - q;
      if (sm::fold(j, n) != q) return false;
    }
  return true;
}

int main(int argc, char** argv) {
  if (argc == 9 && !strcmp(argv[1], "smooth")) {
    const long long H = atoll(argv[3]), W = atoll(argv[4]);
    const int r = atoi(argv[6]), in_place = atoi(argv[7]);
    if (!geometry_holds(H, W)) return 4;
    std::vector<double> plane((size_t)(H * W)), taps((size_t)r + 1), tmp((size_t)(H * W)), out(in_place ? 0 : (size_t)(H * W));
    if (!read_all(argv[2], plane) || !read_all(argv[5], taps)) return 2;
    double* dst = in_place ? plane.data() : out.data();
    if (sm::check_smooth(plane.data(), H, W, taps.data(), r, tmp.data(), dst)) return 5;
    sm::smooth_host(plane.data(), H, W, taps.data(), r, tmp.data(), dst);
    FILE* o = fopen(argv[8], "wb");
    if (!o || !write_some(o, in_place ? plane : out)) return 3;
    fclose(o);
    return 0;
  }
  if (argc == 13 && !strcmp(argv[1], "finish")) {
    const long long Hs = atoll(argv[4]), Ws = atoll(argv[5]), H = atoll(argv[6]), W = atoll(argv[7]);
    const int n_q = atoi(argv[8]), r = atoi(argv[10]);
    const double floor = atof(argv[11]);
    if (!geometry_holds(H, W)) return 4;
    std::vector<uint16_t> rank((size_t)(n_q * Hs * Ws)), valid((size_t)(Hs * Ws));
    std::vector<double> taps((size_t)r + 1);
    std::vector<float> flat((size_t)(H * W)), dark(n_q == 2 ? (size_t)(H * W) : 0);
    if (!read_all(argv[2], rank) || !read_all(argv[3], valid) || !read_all(argv[9], taps)) return 2;
    float* d = n_q == 2 ? dark.data() : nullptr;
    if (sm::check_finish(rank.data(), valid.data(), Hs, Ws, H, W, n_q, taps.data(), r, floor, flat.data(), d)) return 5;
    if (!sm::flat_finish_host(rank.data(), valid.data(), Hs, Ws, H, W, n_q, taps.data(), r, floor, flat.data(), d)) return 6;
    FILE* o = fopen(argv[12], "wb");
    if (!o || !write_some(o, flat) || !write_some(o, dark)) return 3;
    fclose(o);
    return 0;
  }
  fprintf(stderr, "usage: %s smooth plane.raw H W taps.raw radius in_place result.out\n"
                  "       %s finish rank.raw valid.raw Hs Ws H W n_q taps.raw radius floor result.out\n", argv[0], argv[0]);
  return 1;
}
