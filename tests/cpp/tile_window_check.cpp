// tile_window_check.cpp — the windowed tile predicate of csrc/lm_tail_bound.h
// (lm_tb_window + lm_tb_tile_skip_win, what k_tile_bound evaluates) against
// lm_tb_tile_skip (what k_tile_bound_ref evaluates), on the host: a plain
// program, also built with -fsanitize=address,undefined by
// tests/test_tile_window.py.
//
//   tile_window_check
//     For seeded random row-range tables, P_i, N_i and biases: every tile's
//     predicate from the window table of the whole detector, and from the
//     window tables of bands of 1, 2, 7 and 9 tile rows (each band a table of
//     its own whose row 0 is the band's first window row, as in the kernel),
//     must equal lm_tb_tile_skip's.  Covered: oh % 4 in {0, 1, 2, 3}, oh < 4,
//     kh in {1, 2, 16, 30}, 1, 3 and 10 tile columns; the bias is chosen so
//     that U straddles 0 (about half of the tiles skip), and once per table
//     as the negated sum of one tile, so that U is exactly 0 there and a
//     rounding's width away from it in its neighbours.
//     Prints  cases <c> tiles <t> skipped <s> mismatch <m>  and exits 1 on a
//     mismatch or when either outcome never occurred.
//
// Build with -ffp-contract=off, as the library is.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lm_tail_bound.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
double urand() { return (rnd() >> 8) * (1.0 / 16777216.0); }

struct Tally {
  long cases = 0, tiles = 0, skipped = 0, mismatch = 0;
};

// lm_tb_tile_skip's sum without the bias (the same order, in double)
double tile_sum(const std::vector<uint8_t>& rmax, const std::vector<uint8_t>& rmin, int ftx, int oh, int kh, int ty,
                int tx, const double* P, const double* N) {
  const int y0 = ty * LM_TB_H, nr = std::min(y0 + LM_TB_H, oh) - y0;
  double U = 0.0;
  for (int i = 0; i < kh; ++i) {
    unsigned a = 0u, b = 255u;
    for (int r = 0; r < nr; ++r) {
      a = std::max(a, (unsigned)rmax[(size_t)(y0 + i + r) * ftx + tx]);
      b = std::min(b, (unsigned)rmin[(size_t)(y0 + i + r) * ftx + tx]);
    }
    U += P[i] * (double)a - N[i] * (double)b;
  }
  return U;
}

void check(int oh, int kh, int ftx, Tally& T) {
  const int rows = oh + kh - 1, fty = (oh + LM_TB_H - 1) / LM_TB_H;
  std::vector<uint8_t> rmax((size_t)rows * ftx), rmin((size_t)rows * ftx);
  // smooth rows with outliers: windows of four rows then differ from single rows
  for (int r = 0; r < rows; ++r)
    for (int tx = 0; tx < ftx; ++tx) {
      const unsigned lo = rnd() % 40, span = rnd() % 8 == 0 ? rnd() % 216 : rnd() % 30;
      rmin[(size_t)r * ftx + tx] = (uint8_t)lo;
      rmax[(size_t)r * ftx + tx] = (uint8_t)std::min(255u, lo + span);
    }
  std::vector<double> P(kh), N(kh);
  for (int i = 0; i < kh; ++i) {
    P[i] = urand() * 0.01;
    N[i] = urand() * 0.01;
  }
  std::vector<double> sums;
  for (int ty = 0; ty < fty; ++ty)
    for (int tx = 0; tx < ftx; ++tx) sums.push_back(tile_sum(rmax, rmin, ftx, oh, kh, ty, tx, P.data(), N.data()));
  std::vector<double> sorted = sums;
  std::sort(sorted.begin(), sorted.end());
  // biases: the median sum negated (half of the tiles skip), one tile's sum
  // negated exactly, and that a relative 2^-52 to either side
  const double pick = sums[rnd() % sums.size()];
  const double biases[4] = {-sorted[sorted.size() / 2], -pick, -pick * (1.0 + 2.3e-16), -pick * (1.0 - 2.3e-16)};
  for (double bias : biases) {
    ++T.cases;
    // the whole detector as one table, then in bands
    for (int br : {fty, 1, 2, 7, 9}) {
      for (int t0 = 0; t0 < fty; t0 += br) {
        const int t1 = std::min(fty, t0 + br), ohb = std::min(oh, LM_TB_H * t1) - LM_TB_H * t0;
        const int wrows = lm_tb_win_rows(ohb, kh);
        std::vector<uint8_t> wmax((size_t)wrows * ftx), wmin((size_t)wrows * ftx);
        const uint8_t* bmax = rmax.data() + (size_t)LM_TB_H * t0 * ftx;  // the band's window row 0
        const uint8_t* bmin = rmin.data() + (size_t)LM_TB_H * t0 * ftx;
        for (int w = 0; w < wrows; ++w)
          for (int tx = 0; tx < ftx; ++tx)
            lm_tb_window(bmax, bmin, ftx, ohb, kh, w, tx, &wmax[(size_t)w * ftx + tx], &wmin[(size_t)w * ftx + tx]);
        for (int ty = t0; ty < t1; ++ty)
          for (int tx = 0; tx < ftx; ++tx) {
            const bool want =
                lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, kh, ty, tx, P.data(), N.data(), bias);
            const bool got = lm_tb_tile_skip_win(wmax.data(), wmin.data(), ftx, kh, lm_tb_win_row0(ohb, kh, ty - t0), tx,
                                                 P.data(), N.data(), bias);
            ++T.tiles;
            T.skipped += want ? 1 : 0;
            if (got != want) {
              if (T.mismatch < 10)
                printf("mismatch: oh %d kh %d ftx %d band %d tile (%d, %d) bias %.17g: %d, reference %d\n", oh, kh, ftx,
                       br, ty, tx, bias, (int)got, (int)want);
              ++T.mismatch;
            }
          }
      }
    }
  }
}

}  // namespace

int main() {
  Tally T;
  for (int oh : {1, 2, 3, 4, 5, 6, 7, 8, 35, 36, 37, 38, 139, 140})
    for (int kh : {1, 2, 16, 30})
      for (int ftx : {1, 3, 10})
        for (int rep = 0; rep < 3; ++rep) check(oh, kh, ftx, T);
  printf("cases %ld tiles %ld skipped %ld mismatch %ld\n", T.cases, T.tiles, T.skipped, T.mismatch);
  return T.mismatch == 0 && T.skipped > 0 && T.skipped < T.tiles ? 0 : 1;
}
