/*
 * lm_tail_bound.h — an upper bound on a detector's scores over one 40 x 4
 * output tile, from per-row pixel ranges (plain C++: the host runtime's plan lm_tile_plan.h, the
 * k_tile_bound kernels, tests/cpp/tail_bound_check.cpp,
 * tests/cpp/point_bound_check.cpp, tests/cpp/tile_window_check.cpp,
 * tests/cpp/tile_refine_check.cpp, tests/cpp/tile_pair_check.cpp,
 * tests/cpp/tile_sum_rows_check.cpp and tests/cpp/tile_screen_check.cpp share it),
 * its refinement per 8-column output block and tap group (below, lm_tbr_*)
 * and the fp32 screen in front of the refinement's double sum (lm_tbs_*).
 * Written for the tail detectors (hence the name); it serves the point
 * detectors too.
 *
 * The pipeline uses only the sign of a tail score (threshold(> 0), then
 * connected components), and k_ingest zeroes the tail bitmaps, so a tile
 * whose scores are all provably < 0 need not be computed.
 *
 * A point detector's score (paw, snout) is kept only when its mouse pixel is
 * > 25 and the score itself is > 0 (corr_epilogue, lm_corr.hip: the key list
 * takes nothing else), and everything else about it is discarded.  A tile
 * whose scores are all provably < 0 therefore appends no key, whatever its
 * mask pixels are, exactly as a dark tile appends none: the same predicate is
 * sufficient, with the same rounding margin, since the point detectors run
 * the same fp32 chain.
 *
 * The detector: fp32 weights w[i][j] (kh x kw), start value delta, score
 *     s(y, x) = delta + sum_ij w[i][j] I(y + i, x + j)
 * over the window I (u8; output (0, 0) reads I(0 .. kh-1, 0 .. kw-1)).
 *
 * The bound.  Tile (ty, tx) holds the outputs y in [4 ty, y1), x in
 * [40 tx, x1), clipped to oh x ow.  At tap (i, j) every one of them reads a
 * pixel in window rows 4 ty + i .. y1 - 1 + i and columns 40 tx .. x1 - 2 + kw.
 * With M_i / m_i the largest / smallest pixel in that rectangle (here over
 * the column span rounded up to a multiple of LM_TB_BLK, which only widens
 * it), P_i = sum_j max(w[i][j], 0) and N_i = sum_j max(-w[i][j], 0):
 *     s(y, x) <= U = delta + sum_i (P_i M_i - N_i m_i)        (exact arithmetic)
 * since w p <= max(w, 0) M - max(-w, 0) m for every m <= p <= M.
 *
 * Rounding.  The kernels (and the reference) evaluate the score as an fp32
 * chain acc = fl(acc + w p) over n = kh kw taps, fused or as a rounded
 * product and a rounded sum.  By the standard running-error bound the
 * computed value differs from the exact one by at most
 *     gamma_(n+1) (|delta| + sum |w| 255),  gamma_k = k u / (1 - k u), u = 2^-24,
 * plus n underflow errors of at most 2^-126 each; gamma = 2 n 2^-23 = 4 n u
 * covers gamma_(n+1) for n < 2^20.  lm_tb_prepare() adds that, and 1e-6
 * relative for the double evaluation of U and the rounding of P_i / N_i
 * (each off by less than 1e-12 relative), to delta: `bias`.  The tile is
 * skipped iff  bias + sum_i (P_i M_i - N_i m_i) < 0  in double; every
 * computed score of the tile is then < 0.
 * Never skipped: non-finite weights, delta >= 0 or not finite, n >= 2^20,
 * sums beyond 1e30.
 */
#ifndef LM_TAIL_BOUND_H
#define LM_TAIL_BOUND_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_TB_HD __host__ __device__
#else
#define LM_TB_HD
#endif

#define LM_TB_W 40   // tile columns (the dark-tile grid: LM_FW)
#define LM_TB_H 4    // tile rows (LM_FH)
#define LM_TB_BLK 8  // pixel ranges are first taken over aligned blocks of 8 window columns

// P[kh], N[kh] and bias of a detector (row i's weights at w + i * wstride).
// Returns 1 when its tiles may be skipped, 0 when every tile must be computed.
LM_TB_HD inline int lm_tb_prepare(const float* w, int kh, int kw, int wstride, float delta, double* P, double* N,
                                  double* bias) {
  int ok = 1;
  double sabs = 0.0;
  for (int i = 0; i < kh; ++i) {
    double p = 0.0, n = 0.0;
    for (int j = 0; j < kw; ++j) {
      const double v = (double)w[i * wstride + j];
      if (!(v - v == 0.0)) ok = 0;  // NaN or infinite
      if (v > 0.0) p += v;
      else n -= v;
    }
    P[i] = p * (1.0 + 1e-12);  // rounded up
    N[i] = n * (1.0 - 1e-12);  // rounded down (it is subtracted)
    sabs += p + n;
  }
  const double d = (double)delta;
  const double taps = (double)kh * (double)kw;
  const double S = (d < 0.0 ? -d : d) + 255.0 * sabs;
  const double gamma = 2.0 * taps * (1.0 / 8388608.0);  // 2 n 2^-23
  const double margin = gamma * S + 1e-6 * S + taps * 1.2e-38;
  *bias = d + margin;
  if (!(d < 0.0) || !(d - d == 0.0) || !(taps < 1048576.0) || !(S < 1e30)) ok = 0;
  return ok;
}

// Window columns [c0, c1) whose pixels tile column tx's outputs read: from
// 40 tx to the last tap of the last output inside ow, rounded up to a block
// boundary and clipped to the window's ow + kw - 1 columns.
LM_TB_HD inline void lm_tb_span(int tx, int kw, int ow, int* c0, int* c1) {
  const int x1 = (tx + 1) * LM_TB_W < ow ? (tx + 1) * LM_TB_W : ow;
  const int end = (x1 - 1 + kw + LM_TB_BLK - 1) / LM_TB_BLK * LM_TB_BLK;
  *c0 = tx * LM_TB_W;
  *c1 = end < ow + kw - 1 ? end : ow + kw - 1;
}

// The aligned blocks [b0, b1) of LM_TB_BLK view columns that cover window
// columns [c0, c1) of a window whose column 0 is view column x0 >= 0.
// k_tile_bound reduces a view once to pixel ranges per such block for all of
// its detectors, whose windows start at different columns; a detector's span
// is then widened to whole blocks (by < LM_TB_BLK pixels of the same crop row
// on either side), which only weakens the bound.
LM_TB_HD inline void lm_tb_blocks(int x0, int c0, int c1, int* b0, int* b1) {
  *b0 = (x0 + c0) / LM_TB_BLK;
  *b1 = (x0 + c1 + LM_TB_BLK - 1) / LM_TB_BLK;
}

// Largest and smallest pixel of row[c0 .. c1 - 1].
LM_TB_HD inline void lm_tb_row_range(const uint8_t* row, int c0, int c1, uint8_t* mx, uint8_t* mn) {
  unsigned a = 0u, b = 255u;
  for (int c = c0; c < c1; ++c) {
    const unsigned v = row[c];
    a = v > a ? v : a;
    b = v < b ? v : b;
  }
  *mx = (uint8_t)a;
  *mn = (uint8_t)b;
}

// The predicate for tile (ty, tx) from the row ranges rmax / rmin
// ([window row][tile column], ftx tile columns per row): true = every score
// of the tile is < 0.
LM_TB_HD inline bool lm_tb_tile_skip(const uint8_t* rmax, const uint8_t* rmin, int ftx, int oh, int kh, int ty, int tx,
                                     const double* P, const double* N, double bias) {
  const int y0 = ty * LM_TB_H;
  const int nr = (y0 + LM_TB_H < oh ? y0 + LM_TB_H : oh) - y0;  // output rows of the tile inside oh
  double U = bias;
  for (int i = 0; i < kh; ++i) {
    unsigned a = 0u, b = 255u;
    for (int r = 0; r < nr; ++r) {
      const unsigned x = rmax[(y0 + i + r) * ftx + tx], n = rmin[(y0 + i + r) * ftx + tx];
      a = x > a ? x : a;
      b = n < b ? n : b;
    }
    U += P[i] * (double)a - N[i] * (double)b;
  }
  return U < 0.0;
}

// The same predicate from window ranges, which hold the vertical part of
// lm_tb_tile_skip's reduction once instead of once per tile and weight row:
// the LM_TB_H output rows of a tile read, at weight row i, window rows
// 4 ty + i .. 4 ty + i + 3, and that range is the same for every (ty, i) with
// the same 4 ty + i.  A window table for oh output rows (a whole detector, or
// a band of its tile rows whose first window row is row 0) has
//   rows 0 .. lm_tb_win_full(oh, kh) - 1: the range over rows r .. r + 3, for
//     the oh / 4 tile rows of four output rows;
//   then, when oh % 4 != 0, kh rows for the last tile row: row i holds the
//     range over its oh % 4 rows 4 (oh / 4) + i ...
// ftx tile columns per row, as in the row ranges.
LM_TB_HD inline int lm_tb_win_full(int oh, int kh) {
  const int nf = oh / LM_TB_H;
  return nf > 0 ? LM_TB_H * (nf - 1) + kh : 0;
}
LM_TB_HD inline int lm_tb_win_rows(int oh, int kh) {
  return lm_tb_win_full(oh, kh) + (oh % LM_TB_H != 0 ? kh : 0);
}
// Row w of the window table: its first row-range row *r0 and row count *nr.
LM_TB_HD inline void lm_tb_win_src(int oh, int kh, int w, int* r0, int* nr) {
  const int full = lm_tb_win_full(oh, kh);
  if (w < full) {
    *r0 = w;
    *nr = LM_TB_H;
  } else {
    *r0 = oh / LM_TB_H * LM_TB_H + (w - full);
    *nr = oh % LM_TB_H;
  }
}
// The table's first row of tile row ty (weight row i reads that row + i).
LM_TB_HD inline int lm_tb_win_row0(int oh, int kh, int ty) {
  return ty < oh / LM_TB_H ? LM_TB_H * ty : lm_tb_win_full(oh, kh);
}
// Entry (w, tx) of the window table from the row ranges.
LM_TB_HD inline void lm_tb_window(const uint8_t* rmax, const uint8_t* rmin, int ftx, int oh, int kh, int w, int tx,
                                  uint8_t* mx, uint8_t* mn) {
  int r0, nr;
  lm_tb_win_src(oh, kh, w, &r0, &nr);
  unsigned a = 0u, b = 255u;
  for (int r = 0; r < nr; ++r) {
    const unsigned x = rmax[(r0 + r) * ftx + tx], n = rmin[(r0 + r) * ftx + tx];
    a = x > a ? x : a;
    b = n < b ? n : b;
  }
  *mx = (uint8_t)a;
  *mn = (uint8_t)b;
}
// lm_tb_tile_skip from the window table: the tile whose first table row is
// row0 (lm_tb_win_row0), column tx.  The sum runs over i in the same order
// and in double, so the result is lm_tb_tile_skip's.
LM_TB_HD inline bool lm_tb_tile_skip_win(const uint8_t* wmax, const uint8_t* wmin, int ftx, int kh, int row0, int tx,
                                         const double* P, const double* N, double bias) {
  double U = bias;
  for (int i = 0; i < kh; ++i) {
    const unsigned a = wmax[(row0 + i) * ftx + tx], b = wmin[(row0 + i) * ftx + tx];
    U += P[i] * (double)a - N[i] * (double)b;
  }
  return U < 0.0;
}

// ------------------------------------------------------------------------
// The refinement: the same bound per 8-column output block and group of 8
// taps, for the tiles the tile bound fails.  The tile bound takes one pixel
// range per weight row over a tile's whole 40 + kw - 1 columns and four rows,
// so a tile within a detector's reach of an edge sees the full step in every
// row.  Here the outputs are cut into blocks of LM_TB_BLK columns (x0 a
// multiple of 8; 40 is one) and LM_TB_RH rows, and the taps of a weight row
// into groups that end where in_x + j is a multiple of 8 (in_x: the view
// column of the window's column 0, the view being the ext crop whose aligned
// blocks of 8 columns the ranges are taken over): tap j is in group
// (in_x % 8 + j) / 8.  The 8 outputs of a block then read, at the taps of
// group g, view columns 8 (in_x / 8 + g + x0 / 8) .. + 15: two adjacent
// aligned blocks.  With P[i][g] / N[i][g] the sums of the positive and of the
// negated negative weights of row i's group g (rounded as P_i, N_i are) and
// M / m the largest / smallest pixel of those two blocks over the view rows
// in_y + y + i .. + nr - 1 (the second block clipped to the blocks the
// detector's window touches: beyond them no output inside ow reads),
//     U = bias + sum_i sum_g (P[i][g] M - N[i][g] m)
// bounds every score of the block from above, by the argument at the top term
// by term, and bias is the same: the chain's rounding does not depend on how
// the bound is split, and kh (kw + 7) / 8 + kh terms in double stay far inside
// its 1e-6 relative share.  A tile is skipped iff the tile bound proves it or
// every block of it is proven.
// A block proven over four rows is proven in each row: a row's ranges lie
// inside the four rows', so each of its terms is <= the matching term (the
// roundings of the products and of the difference are monotone) and the sums
// run in the same order.  With LM_TB_RH 1 the four-row level is therefore a
// shortcut that never changes a flag (`shortcut`; both forms are kept so that
// a test can compare them).  A last tile row of fewer than four output rows
// uses its own row count.
#ifndef LM_TB_RH
#define LM_TB_RH 4  // rows of an output block at the final level: 1 or 4
#endif
#define LM_TB_NBX (LM_TB_W / LM_TB_BLK)  // output blocks per tile row
static_assert(LM_TB_RH == 1 || LM_TB_RH == LM_TB_H, "block height: a row or a tile");
static_assert(LM_TB_W % LM_TB_BLK == 0, "tiles start on a block boundary");

// Tap groups of a detector row (in_x >= 0) and the taps [*j0, *j1) of group g.
LM_TB_HD inline int lm_tbr_groups(int in_x, int kw) { return (in_x % LM_TB_BLK + kw - 1) / LM_TB_BLK + 1; }
LM_TB_HD inline void lm_tbr_taps(int in_x, int kw, int g, int* j0, int* j1) {
  const int a = in_x % LM_TB_BLK;
  *j0 = LM_TB_BLK * g - a > 0 ? LM_TB_BLK * g - a : 0;
  *j1 = LM_TB_BLK * (g + 1) - a < kw ? LM_TB_BLK * (g + 1) - a : kw;
}
// The group constants of a detector: per weight row i and chunk c of
// LM_TBR_GC groups, LM_TBR_GC values of P (groups GC c ..) and then of N,
// lm_tb_prepare's sums per group; groups past the last hold 0.  (One chunk is
// 64 bytes: a kernel whose detector is uniform fetches it with one scalar
// load.)  lm_tbr_const_size() doubles in all.
#define LM_TBR_GC 4
LM_TB_HD inline int lm_tbr_chunks(int ng) { return (ng + LM_TBR_GC - 1) / LM_TBR_GC; }
LM_TB_HD inline int lm_tbr_const_size(int kh, int ng) { return kh * lm_tbr_chunks(ng) * 2 * LM_TBR_GC; }
LM_TB_HD inline void lm_tbr_prepare(const float* w, int kh, int kw, int wstride, int in_x, double* C) {
  const int ng = lm_tbr_groups(in_x, kw), nc = lm_tbr_chunks(ng);
  for (int i = 0; i < kh; ++i)
    for (int g = 0; g < nc * LM_TBR_GC; ++g) {
      int j0 = 0, j1 = 0;
      if (g < ng) lm_tbr_taps(in_x, kw, g, &j0, &j1);
      double p = 0.0, n = 0.0;
      for (int j = j0; j < j1; ++j) {
        const double v = (double)w[i * wstride + j];
        if (v > 0.0) p += v;
        else if (v < 0.0) n -= v;
      }
      double* q = C + ((i * nc + g / LM_TBR_GC) * 2) * LM_TBR_GC + g % LM_TBR_GC;
      q[0] = p * (1.0 + 1e-12);          // rounded up
      q[LM_TBR_GC] = n * (1.0 - 1e-12);  // rounded down (it is subtracted)
    }
}
// The one definition of a block's sum U: rng(i, g, M, m) yields the largest
// and smallest byte of weight row i's group g (unsigned references).  Every
// user (the host, k_tile_bound_ref, k_tile_bound) goes through it or through
// lm_tbr_sum_rows (below: the same terms in the same order for detectors of
// one chunk per row), so equal ranges give the same bit.
template <class F>
LM_TB_HD inline double lm_tbr_sum(int kh, int ng, const double* C, double bias, F&& rng) {
  static_assert(LM_TBR_GC == 4, "a chunk is read as four P and four N");
  const int nc = lm_tbr_chunks(ng);
  double U = bias;
  // the terms of chunk c of row i, in order; ahead(): the fetch of the next
  // chunk's constants, issued behind this chunk's first ranges (which a
  // kernel has waited for by then) and ahead of its sums
  auto chunk = [&](int i, int c, double p0, double p1, double p2, double p3, double n0, double n1, double n2, double n3,
                   auto&& ahead) {
    const int g = c * LM_TBR_GC, nt = ng - g;
    unsigned M, m;
    rng(i, g, M, m);
    ahead();
    U += p0 * (double)M - n0 * (double)m;
    if (nt > 1) {
      rng(i, g + 1, M, m);
      U += p1 * (double)M - n1 * (double)m;
    }
    if (nt > 2) {
      rng(i, g + 2, M, m);
      U += p2 * (double)M - n2 * (double)m;
    }
    if (nt > 3) {
      rng(i, g + 3, M, m);
      U += p3 * (double)M - n3 * (double)m;
    }
  };
  // The chunks of all rows are contiguous and taken two at a time: a chunk's
  // constants are fetched while the chunk before it is summed, into the
  // registers of the chunk before that.
  const double* q = C;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0, b4 = 0.0, b5 = 0.0, b6 = 0.0, b7 = 0.0;
  int i = 0, c = 0;
  if (kh * nc > 0) a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5], a6 = q[6], a7 = q[7];
  for (int left = kh * nc; left > 0; left -= 2, q += 4 * LM_TBR_GC) {
    chunk(i, c, a0, a1, a2, a3, a4, a5, a6, a7, [&] {
      if (left > 1) b0 = q[8], b1 = q[9], b2 = q[10], b3 = q[11], b4 = q[12], b5 = q[13], b6 = q[14], b7 = q[15];
    });
    if (++c == nc) c = 0, ++i;
    if (left > 1) {
      chunk(i, c, b0, b1, b2, b3, b4, b5, b6, b7, [&] {
        if (left > 2) a0 = q[16], a1 = q[17], a2 = q[18], a3 = q[19], a4 = q[20], a5 = q[21], a6 = q[22], a7 = q[23];
      });
      if (++c == nc) c = 0, ++i;
    }
  }
  return U;
}
// lm_tbr_sum for a detector of one chunk per row (lm_tbr_chunks(ng) == 1: at
// most LM_TBR_GC tap groups, which is every detector up to 25 taps wide and
// the wider ones at a small in_x % 8): row i's constants are the eight doubles
// at C + 8 i, so there is no chunk to count and none to pair; the rows are
// taken two at a time only so that a row's constants are fetched, one row
// ahead, into the registers of the row before it.  The terms, their order and
// their guards (nt = ng) are lm_tbr_sum's: U is the same double bit for bit
// (tests/cpp/tile_sum_rows_check.cpp).  lm_tbr_sum_rows_n: the group count NG
// as a constant, so that a term's guard costs nothing and rng sees which term
// is the row's last (g == NG - 1); lm_tbr_sum_rows chooses among them, and
// takes lm_tbr_sum for any other group count.
template <int NG, class F>
LM_TB_HD inline double lm_tbr_sum_rows_n(int kh, const double* C, double bias, F&& rng) {
  static_assert(LM_TBR_GC == 4 && NG >= 1 && NG <= LM_TBR_GC, "a row is read as four P and four N");
  double U = bias;
  auto row = [&](int i, double p0, double p1, double p2, double p3, double n0, double n1, double n2, double n3,
                 auto&& ahead) {
    unsigned M, m;
    rng(i, 0, M, m);
    ahead();
    U += p0 * (double)M - n0 * (double)m;
    if (NG > 1) {
      rng(i, 1, M, m);
      U += p1 * (double)M - n1 * (double)m;
    }
    if (NG > 2) {
      rng(i, 2, M, m);
      U += p2 * (double)M - n2 * (double)m;
    }
    if (NG > 3) {
      rng(i, 3, M, m);
      U += p3 * (double)M - n3 * (double)m;
    }
  };
  if (kh <= 0) return U;
  const double* q = C;
  double a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5], a6 = q[6], a7 = q[7];
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0, b4 = 0.0, b5 = 0.0, b6 = 0.0, b7 = 0.0;
  for (int i = 0; i < kh; i += 2, q += 4 * LM_TBR_GC) {
    // (past the last row the last row's constants once more: a fetch without a branch)
    const double* qb = q + (i + 1 < kh ? 2 * LM_TBR_GC : 0);
    row(i, a0, a1, a2, a3, a4, a5, a6, a7,
        [&] { b0 = qb[0], b1 = qb[1], b2 = qb[2], b3 = qb[3], b4 = qb[4], b5 = qb[5], b6 = qb[6], b7 = qb[7]; });
    if (i + 1 < kh) {
      const double* qa = qb + (i + 2 < kh ? 2 * LM_TBR_GC : 0);
      row(i + 1, b0, b1, b2, b3, b4, b5, b6, b7,
          [&] { a0 = qa[0], a1 = qa[1], a2 = qa[2], a3 = qa[3], a4 = qa[4], a5 = qa[5], a6 = qa[6], a7 = qa[7]; });
    }
  }
  return U;
}
template <class F>
LM_TB_HD inline double lm_tbr_sum_rows(int kh, int ng, const double* C, double bias, F&& rng) {
  switch (ng) {
    case 1: return lm_tbr_sum_rows_n<1>(kh, C, bias, rng);
    case 2: return lm_tbr_sum_rows_n<2>(kh, C, bias, rng);
    case 3: return lm_tbr_sum_rows_n<3>(kh, C, bias, rng);
    case 4: return lm_tbr_sum_rows_n<4>(kh, C, bias, rng);
    default: return lm_tbr_sum(kh, ng, C, bias, rng);  // (more than one chunk per row, or no group: the generic form)
  }
}
template <class F>
LM_TB_HD inline bool lm_tbr_sum_negative(int kh, int ng, const double* C, double bias, F&& rng) {
  return lm_tbr_sum(kh, ng, C, bias, rng) < 0.0;
}
// ------------------------------------------------------------------------
// The fp32 screen of a block's sum (lm_tbs_*).  Only the sign of U is used,
// and it is almost never close to zero, so a detector of at most LM_TBR_GC tap
// groups is first summed in fp32: two chains a (from the bias) and b (from 0),
//     a <- fma(Pf[i][g], M, a),  b <- fma(-Nf[i][g], m, b)   per term, in lm_tbr_sum's order,
//     U_f = a + b,
// one packed FMA per term on the device.  With the margin E below
//     U_f < -E  =>  U_d < 0 (proven),   U_f >= E  =>  U_d >= 0 (unproven),
// where U_d is lm_tbr_sum's double; only an item with -E <= U_f < E (or a NaN)
// is undecided and takes the double sum, which stays the definition.
//
// The constants (lm_tbs_prepare): Pf the double P[i][g] rounded up to float, Nf
// the double N[i][g] rounded down, bf the double bias rounded up.  The screen is
// off (the double sum alone) when a nonzero constant or the bias is below
// FLT_MIN in magnitude, so every constant used is a normal float or zero and
//     0 <= Pf - P <= 2 u Pf,  0 <= N - Nf <= 2 u N,  0 <= bf - bias <= 2 u |bias|,  u = 2^-24.
// S = |bf| + 255 sum (Pf + Nf), n = kh ng terms.
//
// The margin.  Let U_x = bias + sum (P M - N m) in exact arithmetic.
//  1. Constants.  A pixel range is at most 255, so the exact fp32-constant sum
//     U_fx = bf + sum (Pf M - Nf m) differs from U_x by at most
//     2 u (|bias| + 255 sum (Pf + N)) <= 2 u (1 + 2 u) S.
//  2. The fp32 evaluation.  U_f is a sum of the 2 n + 1 values bf, Pf M, -Nf m
//     by 2 n additions (n per chain and the final one, or any other
//     association of them), each product rounded on its own or fused into its
//     addition: every value passes through at most 2 n additions and one
//     product rounding, so by the running-error bound
//     |U_f - U_fx| <= gamma_(2n+1) S,  gamma_k = k u / (1 - k u) <= 2 k u for k u <= 1/2,
//     which holds for n < 2^20 (the screen is off beyond).  No operation
//     overflows (S < 1e30, or the screen is off).
//  3. Underflow.  The product of a normal constant and an integer >= 1 does
//     not underflow; a sum that falls below FLT_MIN is exact unless it is
//     fused or flushed to zero, and then off by at most 2^-126: 2 n + 1
//     operations, at most (2 n + 1) 2^-126 < (n + 1) 2.4e-38 in all.
//  4. The double sum.  U_d is U_x evaluated in double, each term through at
//     most n + 2 roundings: |U_d - U_x| <= 2 (n + 2) 2^-53 (|bias| + 255 sum (P + N)),
//     and that sum is below (1 + 4 u) S.
// 1 + 2 are below 2 (2 n + 3) u S; the margin is
//     E = 2 (2 n + 4) u S + (1e-12 + (n + 2) 2^-51) S + (n + 1) 2.4e-38,
// whose spare 2 u S covers the second-order parts of 1 and 4 (16 u^2 S and 8 u
// (n + 2) 2^-53 S) and the 1e-12 S the rounding of S and E themselves, computed
// in double and rounded up to float.  Hence |U_f - U_d| <= E for every input.
#define LM_TBS_ROW (2 * LM_TBR_GC)  // floats of a weight row's constants: (Pf_g, -Nf_g) for g = 0 .. 3; one 32-byte scalar load
struct LmTbsConst {
  float bf, E;  // the bias rounded up; the margin
  int on;       // the detector may be screened
};
inline float lm_tbs_up(double x) {  // the smallest float >= x (|x| within the floats' range)
  float f = (float)x;
  return (double)f < x ? nextafterf(f, INFINITY) : f;
}
inline float lm_tbs_down(double x) { return -lm_tbs_up(-x); }
// The screen's constants of a detector from lm_tbr_prepare's C and
// lm_tb_prepare's bias and verdict ok: kh rows of LM_TBS_ROW floats into Cf.
inline LmTbsConst lm_tbs_prepare(const double* C, int kh, int ng, double bias, int ok, float* Cf) {
  LmTbsConst R;
  R.on = ok && ng >= 1 && ng <= LM_TBR_GC ? 1 : 0;
  const double tiny = 1.17549435082228750797e-38;  // FLT_MIN
  double sum = 0.0;
  for (int i = 0; i < kh; ++i)
    for (int g = 0; g < LM_TBR_GC; ++g) {
      const double p = g < ng && R.on ? C[i * 2 * LM_TBR_GC + g] : 0.0, n = g < ng && R.on ? C[(i * 2 + 1) * LM_TBR_GC + g] : 0.0;
      if (!(p - p == 0.0) || !(n - n == 0.0) || (p != 0.0 && p < tiny) || (n != 0.0 && n < tiny) || p > 1e30 || n > 1e30) {
        R.on = 0;
        Cf[i * LM_TBS_ROW + 2 * g] = Cf[i * LM_TBS_ROW + 2 * g + 1] = 0.f;
        continue;
      }
      const float pf = lm_tbs_up(p), nf = lm_tbs_down(n);  // (FLT_MIN is a float: nf is normal or zero as well)
      Cf[i * LM_TBS_ROW + 2 * g] = pf;
      Cf[i * LM_TBS_ROW + 2 * g + 1] = -nf;
      sum += (double)pf + (double)nf;
    }
  const double ab = bias < 0.0 ? -bias : bias;
  if (!(bias - bias == 0.0) || (bias != 0.0 && ab < tiny) || ab > 1e30) {
    R.on = 0;
    R.bf = 0.f;
  } else {
    R.bf = lm_tbs_up(bias);
  }
  const double n = (double)kh * (double)ng, af = R.bf < 0.f ? -(double)R.bf : (double)R.bf;
  const double S = af + 255.0 * sum;
  const double E = (2.0 * (2.0 * n + 4.0) / 16777216.0 + 1e-12 + (n + 2.0) / 2251799813685248.0) * S + (n + 1.0) * 2.4e-38;
  if (!(S < 1e30) || !(n < 1048576.0)) R.on = 0;
  R.E = R.on ? lm_tbs_up(E) : 0.f;
  return R;
}
// Two floats that one packed FMA takes: (a, b) <- (x0 c0 + a, x1 c1 + b), each fused.
#if defined(__clang__)
typedef float lm_tbs_f2 __attribute__((ext_vector_type(2)));
LM_TB_HD inline lm_tbs_f2 lm_tbs_fma2(float x0, float x1, float c0, float c1, lm_tbs_f2 acc) {
  return __builtin_elementwise_fma(lm_tbs_f2{x0, x1}, lm_tbs_f2{c0, c1}, acc);  // v_pk_fma_f32 on the device
}
#else
struct lm_tbs_f2 {
  float x, y;
};
inline lm_tbs_f2 lm_tbs_fma2(float x0, float x1, float c0, float c1, lm_tbs_f2 acc) {
  return lm_tbs_f2{fmaf(x0, c0, acc.x), fmaf(x1, c1, acc.y)};
}
#endif
// U_f of a block for a detector of NG <= LM_TBR_GC tap groups: lm_tbr_sum_rows_n's
// terms in its order (rng as there), the rows two at a time so that a row's
// constants are fetched one row ahead.
template <int NG, class F>
LM_TB_HD inline float lm_tbs_sum_rows_n(int kh, const float* Cf, float bf, F&& rng) {
  static_assert(LM_TBR_GC == 4 && NG >= 1 && NG <= LM_TBR_GC, "a row is read as four pairs");
  lm_tbs_f2 acc = {bf, 0.f};
  auto row = [&](int i, float c0, float c1, float c2, float c3, float c4, float c5, float c6, float c7, auto&& ahead) {
    unsigned M, m;
    rng(i, 0, M, m);
    ahead();
    acc = lm_tbs_fma2((float)M, (float)m, c0, c1, acc);
    if (NG > 1) {
      rng(i, 1, M, m);
      acc = lm_tbs_fma2((float)M, (float)m, c2, c3, acc);
    }
    if (NG > 2) {
      rng(i, 2, M, m);
      acc = lm_tbs_fma2((float)M, (float)m, c4, c5, acc);
    }
    if (NG > 3) {
      rng(i, 3, M, m);
      acc = lm_tbs_fma2((float)M, (float)m, c6, c7, acc);
    }
  };
  if (kh > 0) {
    const float* q = Cf;
    float a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5], a6 = q[6], a7 = q[7];
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, b4 = 0.f, b5 = 0.f, b6 = 0.f, b7 = 0.f;
    for (int i = 0; i < kh; i += 2, q += 2 * LM_TBS_ROW) {
      // (past the last row the last row's constants once more: a fetch without a branch)
      const float* qb = q + (i + 1 < kh ? LM_TBS_ROW : 0);
      row(i, a0, a1, a2, a3, a4, a5, a6, a7,
          [&] { b0 = qb[0], b1 = qb[1], b2 = qb[2], b3 = qb[3], b4 = qb[4], b5 = qb[5], b6 = qb[6], b7 = qb[7]; });
      if (i + 1 < kh) {
        const float* qa = qb + (i + 2 < kh ? LM_TBS_ROW : 0);
        row(i + 1, b0, b1, b2, b3, b4, b5, b6, b7,
            [&] { a0 = qa[0], a1 = qa[1], a2 = qa[2], a3 = qa[3], a4 = qa[4], a5 = qa[5], a6 = qa[6], a7 = qa[7]; });
      }
    }
  }
  return acc.x + acc.y;
}
template <class F>
LM_TB_HD inline float lm_tbs_sum_rows(int kh, int ng, const float* Cf, float bf, F&& rng) {
  switch (ng) {
    case 1: return lm_tbs_sum_rows_n<1>(kh, Cf, bf, rng);
    case 2: return lm_tbs_sum_rows_n<2>(kh, Cf, bf, rng);
    case 3: return lm_tbs_sum_rows_n<3>(kh, Cf, bf, rng);
    default: return lm_tbs_sum_rows_n<4>(kh, Cf, bf, rng);
  }
}
// The decision: -1 proven (U_d < 0), 1 unproven (U_d >= 0), 0 undecided.
LM_TB_HD inline int lm_tbs_decide(float Uf, float E) { return Uf < -E ? -1 : Uf >= E ? 1 : 0; }

// First block (of the view's) that output block xb reads at group 0, and the
// end of the blocks the window touches (nbw: blocks per view row).
LM_TB_HD inline int lm_tbr_block0(int in_x, int xb) { return in_x / LM_TB_BLK + xb; }
LM_TB_HD inline int lm_tbr_block_end(int in_x, int ow, int kw, int nbw) {
  const int e = (in_x + ow + kw - 1 + LM_TB_BLK - 1) / LM_TB_BLK;
  return e < nbw ? e : nbw;
}
// The output block of rows [y, y + nr) and columns [8 xb, 8 xb + 8) from the
// view's block ranges bmax / bmin ([view row][nbw blocks]): true = proven.
LM_TB_HD inline bool lm_tbr_block_skip(const uint8_t* bmax, const uint8_t* bmin, int nbw, int in_y, int in_x, int ow,
                                       int kh, int kw, int y, int nr, int xb, const double* C, double bias) {
  const int b0 = lm_tbr_block0(in_x, xb), bend = lm_tbr_block_end(in_x, ow, kw, nbw);
  return lm_tbr_sum_negative(kh, lm_tbr_groups(in_x, kw), C, bias, [&](int i, int g, unsigned& M, unsigned& m) {
    const int ba = b0 + g, bb = ba + 1 < bend ? ba + 1 : bend - 1;
    M = 0u;
    m = 255u;
    for (int r = 0; r < nr; ++r) {
      const int row = (in_y + y + i + r) * nbw;
      const unsigned xa = bmax[row + ba], xb2 = bmax[row + bb], na = bmin[row + ba], nb = bmin[row + bb];
      M = xa > M ? xa : M;
      M = xb2 > M ? xb2 : M;
      m = na < m ? na : m;
      m = nb < m ? nb : m;
    }
  });
}
// The screen's decision (lm_tbs_decide) for the same block from the same
// ranges: the host form of what k_tile_bound computes first, term for term.
LM_TB_HD inline int lm_tbs_block(const uint8_t* bmax, const uint8_t* bmin, int nbw, int in_y, int in_x, int ow, int kh,
                                 int kw, int y, int nr, int xb, const float* Cf, float bf, float E) {
  const int b0 = lm_tbr_block0(in_x, xb), bend = lm_tbr_block_end(in_x, ow, kw, nbw);
  const float Uf = lm_tbs_sum_rows(kh, lm_tbr_groups(in_x, kw), Cf, bf, [&](int i, int g, unsigned& M, unsigned& m) {
    const int ba = b0 + g, bb = ba + 1 < bend ? ba + 1 : bend - 1;
    M = 0u;
    m = 255u;
    for (int r = 0; r < nr; ++r) {
      const int row = (in_y + y + i + r) * nbw;
      const unsigned xa = bmax[row + ba], xb2 = bmax[row + bb], na = bmin[row + ba], nb = bmin[row + bb];
      M = xa > M ? xa : M;
      M = xb2 > M ? xb2 : M;
      m = na < m ? na : m;
      m = nb < m ? nb : m;
    }
  });
  return lm_tbs_decide(Uf, E);
}
// ------------------------------------------------------------------------
// Range tables as k_tile_bound keeps them: one 16-bit entry M | m << 8 per
// (row, block), two entries (blocks 2 w and 2 w + 1) per 32-bit word, an even
// number nbk of blocks per row.  lm_tb_range_merge: the range over two words'
// blocks, entry by entry (the largest of bytes 0 and 2, the smallest of bytes
// 1 and 3).
LM_TB_HD inline uint32_t lm_tb_range_merge(uint32_t a, uint32_t b) {
  const uint32_t a0 = a & 0xFFu, b0 = b & 0xFFu, a1 = a & 0xFF00u, b1 = b & 0xFF00u;
  const uint32_t a2 = a & 0xFF0000u, b2 = b & 0xFF0000u, a3 = a & 0xFF000000u, b3 = b & 0xFF000000u;
  return (a0 > b0 ? a0 : b0) | (a1 < b1 ? a1 : b1) | (a2 > b2 ? a2 : b2) | (a3 < b3 ? a3 : b3);
}
// The pair table of a range table: entry b of a row is the range over blocks
// b and b + 1 of that row, which is what a term of the refinement reads (the
// last block of the row stands alone).  Word w of a row from the table's words
// w and w + 1 (last: w is the row's last word, there is no w + 1).
LM_TB_HD inline uint32_t lm_tbr_pair_word(uint32_t w, uint32_t wnext, bool last) {
  return lm_tb_range_merge(w, (w >> 16) | (last ? w & 0xFFFF0000u : wnext << 16));
}
// The range a term reads at block ba of a detector whose window ends before
// block bendl (the second block is clipped to bendl - 1: at ba == bendl - 1
// the term sees block ba alone, whatever the table holds beyond it).  plain,
// pair: the row's entries of the range table and of its pair table; pair
// null: the pair is formed from plain.
LM_TB_HD inline void lm_tbr_pair_range(const uint16_t* pair, const uint16_t* plain, int ba, int bendl, unsigned& M,
                                       unsigned& m) {
  if (pair != nullptr) {
    const unsigned q = ba == bendl - 1 ? plain[ba] : pair[ba];
    M = q & 0xFFu;
    m = q >> 8;
  } else {
    const unsigned qa = plain[ba], qb = plain[ba + 1 < bendl ? ba + 1 : bendl - 1];
    M = (qa & 0xFFu) > (qb & 0xFFu) ? qa & 0xFFu : qb & 0xFFu;
    m = (qa >> 8) < (qb >> 8) ? qa >> 8 : qb >> 8;
  }
}
// The same for the LM_TBR_GC terms of a chunk at once, as k_tile_bound reads
// them: w0 .. w2 are the pair table's words ba / 2 .. ba / 2 + 2 of the row
// (ba: the block of the chunk's first term; they cover the entries ba .. ba +
// 3 at either parity, and the words past a row's last block are never used),
// x0 / x1 receive entries ba, ba + 1 / ba + 2, ba + 3.  lm_tbr_quad_get:
// term j of the chunk; clip: this term stands at block bendl - 1, `alone` is
// the plain table's entry there.
LM_TB_HD inline void lm_tbr_quad_align(uint32_t w0, uint32_t w1, uint32_t w2, int ba, uint32_t& x0, uint32_t& x1) {
  const int s = 16 * (ba & 1);
  x0 = (uint32_t)(((uint64_t)w1 << 32 | w0) >> s);
  x1 = (uint32_t)(((uint64_t)w2 << 32 | w1) >> s);
}
LM_TB_HD inline void lm_tbr_quad_get(uint32_t x0, uint32_t x1, int j, bool clip, unsigned alone, unsigned& M,
                                     unsigned& m) {
  const unsigned q = clip ? alone : ((j & 2 ? x1 : x0) >> (16 * (j & 1))) & 0xFFFFu;
  M = q & 0xFFu;
  m = q >> 8;
}

// The tile rule's second half for tile (ty, tx): every block proven at block
// height rh (1 or LM_TB_H).
LM_TB_HD inline bool lm_tbr_tile_skip(const uint8_t* bmax, const uint8_t* bmin, int nbw, int in_y, int in_x, int oh,
                                      int ow, int kh, int kw, int ty, int tx, const double* C, double bias, int rh,
                                      bool shortcut) {
  const int y0 = ty * LM_TB_H;
  const int nr = (y0 + LM_TB_H < oh ? y0 + LM_TB_H : oh) - y0;
  const int nbx = (ow + LM_TB_BLK - 1) / LM_TB_BLK;
  for (int xb = tx * LM_TB_NBX; xb < (tx + 1) * LM_TB_NBX && xb < nbx; ++xb) {
    if (rh != 1) {
      if (!lm_tbr_block_skip(bmax, bmin, nbw, in_y, in_x, ow, kh, kw, y0, nr, xb, C, bias)) return false;
      continue;
    }
    if (shortcut && nr == LM_TB_H &&
        lm_tbr_block_skip(bmax, bmin, nbw, in_y, in_x, ow, kh, kw, y0, nr, xb, C, bias))
      continue;
    for (int r = 0; r < nr; ++r)
      if (!lm_tbr_block_skip(bmax, bmin, nbw, in_y, in_x, ow, kh, kw, y0 + r, 1, xb, C, bias)) return false;
  }
  return true;
}

#endif  // LM_TAIL_BOUND_H
