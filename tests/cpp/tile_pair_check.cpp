// tile_pair_check.cpp — the paired block ranges of csrc/lm_tail_bound.h (the
// pair table a term of the refinement reads in k_tile_bound: entry b of a row
// is the range over blocks b and b + 1) on the host: a plain program, also
// built with -fsanitize=address,undefined by tests/test_tile_pairs.py.
//
// From random block ranges of a view (with rows of equal bytes and blocks of
// 0 and 255) it builds what a band of k_tile_bound holds -- the block ranges
// B of the columns the detectors' windows touch (an even first block, an even
// count), their four-row windows V, the windows' pair table -- with the
// header's own functions, and evaluates every output block of a tile row of
// two detectors of the view (a wide one, and a narrower one that shares its
// centre column, so that its window ends in an earlier block) the way the
// kernel does: four rows from the pair table, a chunk of four terms from
// three words (lm_tbr_quad_*), fetched a chunk ahead, which may lie past the
// row's or the table's end (a spare row, filled with a pattern here) and then
// must not be used; fewer rows from
// B, the pairs formed on the way.  Every term's M, m must be what
// lm_tbr_block_skip takes from the view's ranges (restated here: blocks ba and
// min(ba + 1, bend - 1) over the rows), through lm_tbr_pair_range as well, and
// lm_tbr_sum_negative through the accessors must return lm_tbr_block_skip's
// value.
//
// Geometries: kw 9 .. 70 x every in_x mod 8 x windows that end on a block
// boundary, one column and seven columns past it x 1 .. 4 rows.  Prints
//   <n> geometries, <b> blocks, <p> proven, <t> terms, <c> clipped, <e> earlier, <f> failures
// (clipped: terms at the window's last block, which stand alone; earlier:
// those of them with a block of the table beyond).
//
// Build with -ffp-contract=off, as the library is.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lm_tail_bound.h"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Tally {
  long geoms = 0, blocks = 0, proven = 0, terms = 0, clipped = 0, earlier = 0, fails = 0;
};

struct DetGeom {
  int kh, kw, in_y, in_x, oh, ow;
};

void fail(Tally& T, const char* what, const DetGeom& D, int xb, int i, int g) {
  if (T.fails++ < 10)
    std::printf("FAIL %s: kh %d kw %d in (%d, %d) out %d x %d block %d row %d group %d\n", what, D.kh, D.kw, D.in_y, D.in_x,
                D.oh, D.ow, xb, i, g);
}

// One view: eh rows of nbw blocks; two detectors; nr output rows in the tile row checked.
void run_view(Rng& R, int kw, int xm, int endmod, int nr, Tally& T) {
  const int kh = 3 + R.below(3), kwn = std::max(2, kw - 2 * (4 + R.below(8)));
  // the wide detector's window starts at in_x (in_x mod 8 = xm), the narrow one's kw / 2 - kwn / 2 further in
  DetGeom D[2];
  const int in_x = 8 * R.below(3) + xm, in_y = R.below(3);
  // outputs: the wide window ends endmod columns past a block boundary (in_x + ow + kw - 1 = endmod mod 8)
  int ow = 41 + R.below(48);
  while ((in_x + ow + kw - 1) % 8 != endmod) ++ow;
  const int y0 = 4, oh = y0 + nr;  // the second tile row is the last, of nr rows
  D[0] = {kh, kw, in_y, in_x, oh, ow};
  D[1] = {kh, kwn, in_y + R.below(2), in_x + kw / 2 - kwn / 2, oh, ow};
  int eh = 0, ewn = 0;
  for (const DetGeom& d : D) {
    eh = std::max(eh, d.in_y + d.oh + d.kh - 1);
    ewn = std::max(ewn, d.in_x + d.ow + d.kw - 1);
  }
  const int ew = (ewn + 15) / 16 * 16 + 16 * R.below(2), nbw = ew / LM_TB_BLK;
  // the view's block ranges
  std::vector<uint8_t> bmax((size_t)eh * nbw), bmin((size_t)eh * nbw);
  for (int r = 0; r < eh; ++r) {
    const int mode = R.below(4);  // a row of random ranges, of equal bytes, of 0 / 255 blocks, mixed
    for (int b = 0; b < nbw; ++b) {
      int a = R.below(256), c = R.below(256);
      const int m = mode == 3 ? R.below(3) : mode;
      if (m == 1) c = a;
      if (m == 2) a = R.below(2) ? 255 : 0, c = R.below(2) ? a : (R.below(2) ? 255 : 0);
      bmax[(size_t)r * nbw + b] = (uint8_t)std::max(a, c);
      bmin[(size_t)r * nbw + b] = (uint8_t)std::min(a, c);
    }
  }
  // the band's tables: blocks blo .. blo + nbk of all rows (both even, as the runtime lays them out)
  int b_lo = nbw, b_hi = 0;
  for (const DetGeom& d : D) {
    b_lo = std::min(b_lo, d.in_x / LM_TB_BLK);
    b_hi = std::max(b_hi, (d.in_x + d.ow + d.kw - 1 + LM_TB_BLK - 1) / LM_TB_BLK);
  }
  const int blo = b_lo / 2 * 2, nbk = std::min((b_hi + 1) / 2 * 2, nbw) - blo, nw = nbk / 2;
  const uint32_t kPattern = 0x5AA5C33Cu;  // what lies past a table
  std::vector<uint32_t> B((size_t)eh * nw), V((size_t)std::max(0, eh - 3) * nw), VP(V.size() + nw + 3, kPattern);
  for (int r = 0; r < eh; ++r)
    for (int w = 0; w < nw; ++w) {
      const size_t e = (size_t)r * nbw + blo + 2 * w;
      B[(size_t)r * nw + w] = (uint32_t)bmax[e] | (uint32_t)bmin[e] << 8 | (uint32_t)bmax[e + 1] << 16 | (uint32_t)bmin[e + 1] << 24;
    }
  for (size_t e = 0; e < V.size(); ++e)
    V[e] = lm_tb_range_merge(lm_tb_range_merge(B[e], B[e + nw]), lm_tb_range_merge(B[e + 2 * nw], B[e + 3 * nw]));
  for (size_t e = 0; e < V.size(); ++e) {
    const bool last = (int)(e % nw) == nw - 1;
    VP[e] = lm_tbr_pair_word(V[e], last ? 0u : V[e + 1], last);
  }
  // (entries as the kernel reads them: two per word, the even block in the low half)
  std::vector<uint16_t> B16(2 * B.size()), V16(2 * V.size()), P16(2 * VP.size());
  for (size_t e = 0; e < B.size(); ++e) B16[2 * e] = (uint16_t)B[e], B16[2 * e + 1] = (uint16_t)(B[e] >> 16);
  for (size_t e = 0; e < V.size(); ++e) V16[2 * e] = (uint16_t)V[e], V16[2 * e + 1] = (uint16_t)(V[e] >> 16);
  for (size_t e = 0; e < VP.size(); ++e) P16[2 * e] = (uint16_t)VP[e], P16[2 * e + 1] = (uint16_t)(VP[e] >> 16);

  for (const DetGeom& d : D) {
    ++T.geoms;
    const int ng = lm_tbr_groups(d.in_x, d.kw), nc = lm_tbr_chunks(ng);
    std::vector<float> w((size_t)d.kh * d.kw);
    for (float& x : w) x = (float)(R.below(2001) - 1000) / 1000.0f;
    std::vector<double> C((size_t)lm_tbr_const_size(d.kh, ng));
    lm_tbr_prepare(w.data(), d.kh, d.kw, d.kw, d.in_x, C.data());
    const int bend = lm_tbr_block_end(d.in_x, d.ow, d.kw, nbw), bendl = bend - blo;
    const int bl0 = lm_tbr_block0(d.in_x, 0) - blo, nbx = (d.ow + LM_TB_BLK - 1) / LM_TB_BLK;
    // the windows' entries at the last block of the detector's window (one spare), kept apart as the kernel keeps them
    std::vector<uint16_t> AL(V.size() / nw + 1, (uint16_t)kPattern);
    for (size_t r = 0; r < V.size() / nw; ++r) AL[r] = V16[r * nbk + bendl - 1];
    const int row0 = d.in_y + (nr == LM_TB_H ? 0 : y0);  // four rows: the first tile row; fewer: the last
    const int y = nr == LM_TB_H ? 0 : y0;
    // a bias that cancels the sum of the middle block but for a little, so that both outcomes occur
    double mid = 0.0;
    for (int i = 0; i < d.kh; ++i)
      for (int g = 0; g < ng; ++g) {
        const double* q = C.data() + ((i * nc + g / LM_TBR_GC) * 2) * LM_TBR_GC + g % LM_TBR_GC;
        const int ba = lm_tbr_block0(d.in_x, nbx / 2) + g, bb = ba + 1 < bend ? ba + 1 : bend - 1;
        unsigned M = 0u, m = 255u;
        for (int r = 0; r < nr; ++r) {
          const size_t row = (size_t)(d.in_y + y + i + r) * nbw;
          M = std::max({M, (unsigned)bmax[row + ba], (unsigned)bmax[row + bb]});
          m = std::min({m, (unsigned)bmin[row + ba], (unsigned)bmin[row + bb]});
        }
        mid += q[0] * (double)M - q[LM_TBR_GC] * (double)m;
      }
    const double bias = -mid + (double)(R.below(2001) - 1000) * 0.01;
    for (int xb = 0; xb < nbx; ++xb) {
      const int ba0 = bl0 + xb;
      // the ranges lm_tbr_block_skip takes
      auto expect = [&](int i, int g, unsigned& M, unsigned& m) {
        const int ba = lm_tbr_block0(d.in_x, xb) + g, bb = ba + 1 < bend ? ba + 1 : bend - 1;
        M = 0u;
        m = 255u;
        for (int r = 0; r < nr; ++r) {
          const size_t row = (size_t)(d.in_y + y + i + r) * nbw;
          M = std::max({M, (unsigned)bmax[row + ba], (unsigned)bmax[row + bb]});
          m = std::min({m, (unsigned)bmin[row + ba], (unsigned)bmin[row + bb]});
        }
      };
      auto check = [&](const char* what, int i, int g, unsigned M, unsigned m) {
        unsigned M0, m0;
        expect(i, g, M0, m0);
        if (M != M0 || m != m0) fail(T, what, d, xb, i, g);
      };
      const bool want = lm_tbr_block_skip(bmax.data(), bmin.data(), nbw, d.in_y, d.in_x, d.ow, d.kh, d.kw, y, nr, xb,
                                          C.data(), bias);
      ++T.blocks;
      T.proven += want ? 1 : 0;
      bool got, got2;
      if (nr == LM_TB_H) {
        // as k_tile_bound's four-row level: a chunk's words fetched ahead, the last group's block read alone
        const uint32_t* pw = VP.data() + (size_t)row0 * nw + (ba0 >> 1);
        const uint16_t* alone = AL.data() + row0;
        const bool clipped = ba0 + ng == bendl;
        const int jl = (ng - 1) % LM_TBR_GC;
        uint32_t w0, w1, w2, x0 = 0u, x1 = 0u;
        unsigned qn, q = 0u;
        bool lastc = false;
        auto fetch = [&]() {
          w0 = pw[0];
          w1 = pw[1];
          w2 = pw[2];
          qn = *alone;
        };
        fetch();
        got = lm_tbr_sum_negative(d.kh, ng, C.data(), bias, [&](int i, int g, unsigned& M, unsigned& m) {
          if (g % LM_TBR_GC == 0) {
            const int c = g / LM_TBR_GC;
            lm_tbr_quad_align(w0, w1, w2, ba0, x0, x1);
            q = qn;
            lastc = c == nc - 1;
            pw += lastc ? nw - 2 * (nc - 1) : 2;  // (after the last chunk: the spare row)
            alone += lastc ? 1 : 0;
            fetch();
          }
          lm_tbr_quad_get(x0, x1, g % LM_TBR_GC, lastc && clipped && g % LM_TBR_GC == jl, q, M, m);
          check("chunk of the pair table", i, g, M, m);
          ++T.terms;
          if (ba0 + g == bendl - 1) {
            ++T.clipped;
            T.earlier += bendl < nbk ? 1 : 0;
            if (g != ng - 1) fail(T, "the window's last block at another group than the last", d, xb, i, g);
          }
        });
        got2 = lm_tbr_sum_negative(d.kh, ng, C.data(), bias, [&](int i, int g, unsigned& M, unsigned& m) {
          lm_tbr_pair_range(P16.data() + (size_t)(row0 + i) * nbk, V16.data() + (size_t)(row0 + i) * nbk, ba0 + g, bendl, M, m);
          check("pair table", i, g, M, m);
        });
      } else {
        // as its level over fewer rows: pairs formed from B, row by row
        auto level_b = [&](const char* what) {
          return lm_tbr_sum_negative(d.kh, ng, C.data(), bias, [&](int i, int g, unsigned& M, unsigned& m) {
            const uint16_t* row = B16.data() + (size_t)(row0 + i) * nbk;
            M = 0u;
            m = 255u;
            for (int r = 0; r < nr; ++r, row += nbk) {
              unsigned a, b;
              lm_tbr_pair_range(nullptr, row, ba0 + g, bendl, a, b);
              M = std::max(M, a);
              m = std::min(m, b);
            }
            check(what, i, g, M, m);
            ++T.terms;
            if (ba0 + g == bendl - 1) {
              ++T.clipped;
              T.earlier += bendl < nbk ? 1 : 0;
            }
          });
        };
        got = level_b("pairs from the block ranges");
        got2 = got;
      }
      if (got != want || got2 != want) fail(T, "lm_tbr_sum_negative's value", d, xb, -1, -1);
    }
  }
}

}  // namespace

int main() {
  Rng R{20240611u};
  Tally T;
  static const int kEnds[3] = {0, 1, 7};
  for (int kw = 9; kw <= 70; ++kw)
    for (int xm = 0; xm < LM_TB_BLK; ++xm)
      for (int endmod : kEnds)
        for (int nr = 1; nr <= LM_TB_H; ++nr) run_view(R, kw, xm, endmod, nr, T);
  std::printf("%ld geometries, %ld blocks, %ld proven, %ld terms, %ld clipped, %ld earlier, %ld failures\n", T.geoms, T.blocks,
              T.proven, T.terms, T.clipped, T.earlier, T.fails);
  return T.fails == 0 ? 0 : 1;
}
