// calib_core_check.cpp — csrc/lm_calib_core.h on the host against a
// brute-force statement, as a stand-alone program (built with
// -fsanitize=address,undefined by tests/test_calib.py): the per-view record on
// random small frames (every pixel of the view tested for the peak, the count
// and membership of the window, tight buffers so that a read outside the frame
// is caught), and the fit on random polynomials with planted outliers (the
// outliers and the clipped frames dropped, the polynomial recovered, the map
// inside the frame).  Exits 0 and prints "<n> cases, 0 failures".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lm_calib_core.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static double unit() { return (double)(rnd() >> 8) / (double)(1u << 24); }

static int check_record(int c) {
  const int rows = 2 + (int)(rnd() % 9), cols = 1 + (int)(rnd() % 40), split = 1 + (int)(rnd() % (rows - 1));
  lm_calib_opts o{(int32_t)(rnd() % 120), (int32_t)(rnd() % 7), 80, 1, 8, 0};
  if (c % 9 == 0) o.radius = 50;  // larger than the frame
  const size_t npix = (size_t)rows * cols;
  std::vector<uint8_t> F(npix), B(npix);
  const uint32_t kind = rnd() % 5;
  for (size_t i = 0; i < npix; ++i) {
    B[i] = (uint8_t)(kind == 0 ? 0 : rnd() % 64);
    switch (kind) {
      case 0: F[i] = 255; break;                                       // saturated
      case 1: F[i] = (uint8_t)(B[i] / 2); break;                        // darker than the background
      case 2: F[i] = (uint8_t)(B[i] + (rnd() % 4 ? 0 : 150)); break;    // many equal peaks
      case 3: F[i] = (uint8_t)(B[i] + o.threshold + rnd() % 2); break;  // at and just above the threshold
      default: F[i] = (uint8_t)(rnd() & 255); break;
    }
  }
  int bad = 0;
  for (int view = 0; view < 2; ++view) {
    lm_calib_record got;
    lmc_host_record(F.data(), B.data(), rows, cols, split, view, o, &got);
    const int r0 = view ? split : 0, r1 = view ? rows : split;
    int peak = -1, px = 0, py = 0, above = 0;
    for (int r = r0; r < r1; ++r)
      for (int x = 0; x < cols; ++x) {
        const int d = std::max(0, (int)F[(size_t)r * cols + x] - (int)B[(size_t)r * cols + x]);
        if (d > peak) peak = d, px = x, py = r;
        above += d > o.threshold;
      }
    lm_calib_record want{};
    want.peak = peak, want.px = px, want.py = py, want.n_above = above;
    for (int dr = -o.radius; dr <= o.radius; ++dr)
      for (int dc = -o.radius; dc <= o.radius; ++dc) {
        const int r = py + dr, x = px + dc;
        if (r < r0 || r >= r1 || x < 0 || x >= cols) {
          want.clipped = 1;
          continue;
        }
        const int d = std::max(0, (int)F[(size_t)r * cols + x] - (int)B[(size_t)r * cols + x]);
        if (d > o.threshold) want.n_in += 1, want.S += d, want.Sx += (int64_t)d * x, want.Sy += (int64_t)d * r;
      }
    if (got.peak != want.peak || got.px != want.px || got.py != want.py || got.n_above != want.n_above ||
        got.n_in != want.n_in || got.clipped != want.clipped || got.S != want.S || got.Sx != want.Sx || got.Sy != want.Sy) {
      ++bad;
      printf("case %d view %d (%d x %d split %d R %d thr %d): peak %d/%d at %d,%d / %d,%d n_above %d/%d n_in %d/%d clipped %d/%d\n",
             c, view, rows, cols, split, o.radius, o.threshold, got.peak, want.peak, got.px, got.py, want.px, want.py,
             got.n_above, want.n_above, got.n_in, want.n_in, got.clipped, want.clipped);
    }
  }
  return bad;
}

static int check_fit(int c) {
  const int cols = 200 + (int)(rnd() % 1800), degree = 1 + (int)(rnd() % 3), n = 16 * (degree + 1) + 8 + (int)(rnd() % 60);
  lm_calib_opts o{40, 12, 80, 12, 8, 0};
  double truth[4] = {0.5 * cols + 20 * (unit() - 0.5), 0.5 * cols * (0.9 + 0.2 * unit()), 6 * (unit() - 0.5), 4 * (unit() - 0.5)};
  for (int k = degree + 1; k < 4; ++k) truth[k] = 0;
  std::vector<lm_calib_record> rec((size_t)n * 2);
  int outliers = 0, blanks = 0;
  for (int f = 0; f < n; ++f) {
    const double xb = 0.1 * cols + 0.8 * cols * (f + unit()) / n;
    double xs = lmc_poly(truth, degree, lmc_t(xb, cols));
    const bool out = f % 17 == 8 && 4 * f > n && 4 * f < 3 * n, blank = f % 13 == 7;  // (outliers away from the ends)
    if (out) xs += (outliers % 2 ? 5.0 : -5.0), ++outliers;
    for (int view = 0; view < 2; ++view) {
      lm_calib_record& r = rec[(size_t)2 * f + view];
      const int64_t S = 1 << 30;  // (coordinates exact to 2^-30)
      r = lm_calib_record{200, 0, 0, 30, 30, 0, S, (int64_t)llround((view ? xb : xs) * (double)S), 0};
      if (blank && view == (f & 1)) r.clipped = 1;
    }
    if (blank) ++blanks, outliers -= out;
  }
  lm_calib_fit_result res;
  const std::string why = lmc_fit(rec.data(), n, cols, o, degree, 1.5, &res);
  int bad = 0;
  if (!why.empty()) {
    printf("fit case %d: refused: %s\n", c, why.c_str());
    return 1;
  }
  if (res.n_frames != n || res.n_samples != n - blanks || res.n_used != n - blanks - outliers) ++bad;
  for (int f = 0; f < n && !bad; ++f) {
    const double xb = (double)rec[(size_t)2 * f + 1].Sx / (double)rec[(size_t)2 * f + 1].S;
    if (fabs(lmc_poly(res.coef, degree, lmc_t(xb, cols)) - lmc_poly(truth, degree, lmc_t(xb, cols))) > 1e-5) ++bad;
  }
  if (!(res.rms < 1e-5) || !(res.max_abs_resid < 1e-5) || !(res.lo >= 0.1 * cols) || !(res.hi <= 0.9 * cols)) ++bad;
  std::vector<int32_t> map((size_t)4 * cols);
  int32_t boxes[8];
  const std::string whym = lmc_map(res, 4, cols, 2, map.data(), boxes);
  if (!whym.empty()) ++bad;
  for (int x = 0; x < cols && whym.empty(); ++x)
    if (map[(size_t)x] < 0 || map[(size_t)x] >= cols || map[(size_t)3 * cols + x] != 3 * cols + x) ++bad;
  if (bad)
    printf("fit case %d (cols %d degree %d n %d): samples %d used %d (want %d, %d) rms %g worst %g %s\n", c, cols, degree, n,
           res.n_samples, res.n_used, n - blanks, n - blanks - outliers, res.rms, res.max_abs_resid, whym.c_str());
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  const int cases = argc > 1 ? atoi(argv[1]) : 300;
  if (argc > 2) g_state ^= strtoull(argv[2], nullptr, 10);
  int failures = 0;
  for (int c = 0; c < cases; ++c) failures += check_record(c) + check_fit(c);
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
