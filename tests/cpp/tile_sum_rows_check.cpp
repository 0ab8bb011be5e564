// tile_sum_rows_check.cpp — the two forms of a block's sum (csrc/
// lm_tail_bound.h: lm_tbr_sum, lm_tbr_sum_rows) and the order "end blocks
// first" over a tile's blocks (round_block below; measured in k_tile_bound and
// not kept there) on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_tile_sum_rows.py.
//
//   tile_sum_rows_check sums
//     Detectors of one chunk per row: random weights through lm_tbr_prepare,
//     kh 1 .. 40, 1 .. 4 tap groups at every in_x % 8, random byte ranges per
//     (row, group).  lm_tbr_sum_rows must return lm_tbr_sum's U bit for bit,
//     at the detector's own bias and at biases of the negated sum of the terms
//     moved by -3 .. 3 ulps (the sign test at zero).  Prints
//       <n> cases, <s> sums, <neg> negative, <z> zero, <pos> positive, <c> calls differ, <f> failures
//   tile_sum_rows_check rounds
//     Synthetic detectors and images with last tile columns of 1 .. 5 blocks
//     (ow % 40 of 8, 16, 24, 32, 0 and ow no multiple of 8): the block flags of
//     lm_tbr_block_skip replayed in the two-round order must mark a tile
//     exactly when lm_tbr_tile_skip keeps it, and every block must be the item
//     of exactly one round.  Prints
//       <t> tiles, <e> kept by an end, <m> kept by a middle block only, <p> proven, <c> short columns, <f> failures
//   tile_sum_rows_check views FILE
//     Recorded views (written by the test: per detector ten int32 -- kh, kw,
//     oh, ow, frames, eh, ew, in_y, in_x, kind -- the start value, the weights,
//     then the views' bytes): the block sums each order needs over the tiles
//     the tile bound fails.  Prints per detector
//       det <d>: refined <r> kept <k> ends <e> all <a> ends_first <b> sequential <s> short <c> failures <f>
//     (ends: kept by an end block; short: refined tiles of a last tile column of fewer than five blocks)
//
// Build with -ffp-contract=off, as the library is built.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_tail_bound.h"

namespace {

// The tile rule is an OR over a tile's blocks (kept as soon as one block is
// unproven), so the order in which they are tried is free.  Two rounds: the
// first and the last of the tile's nb existing blocks (a last tile column has
// fewer than LM_TB_NBX), then, only for a tile that neither marked, the blocks
// between them.  round_block: the block of item q (0 .. round_items(rd) - 1)
// of round rd (0, 1), or nb when the tile has no such block (one block is one
// item of round 0, two blocks leave none for round 1).
int round_items(int rd) { return rd == 0 ? 2 : LM_TB_NBX - 2; }
int round_block(int rd, int q, int nb) {
  if (rd == 0) return q == 0 ? 0 : nb > 1 ? nb - 1 : nb;
  return q + 1 < nb - 1 ? q + 1 : nb;
}

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t next64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
double uniform() { return (double)(next64() >> 11) / 9007199254740992.0; }  // [0, 1)
int below(int n) { return (int)(uniform() * n); }

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int run_sums() {
  long cases = 0, sums = 0, neg = 0, zero = 0, pos = 0, calls = 0, fails = 0;
  for (int kh = 1; kh <= 40; ++kh)
    for (int ng = 1; ng <= LM_TBR_GC; ++ng)
      for (int a = 0; a < LM_TB_BLK; ++a) {
        // the widths with ng tap groups at this residue: 8 (ng - 1) - a < kw <= 8 ng - a
        const int lo = LM_TB_BLK * (ng - 1) - a + 1 > 1 ? LM_TB_BLK * (ng - 1) - a + 1 : 1, hi = LM_TB_BLK * ng - a;
        if (hi < lo) continue;
        const int kw = lo + below(hi - lo + 1), in_x = a + LM_TB_BLK * below(3);
        if (lm_tbr_groups(in_x, kw) != ng || lm_tbr_chunks(ng) != 1) {
          ++fails;
          printf("FAIL: kw %d at in_x %d has %d groups, not %d\n", kw, in_x, lm_tbr_groups(in_x, kw), ng);
          continue;
        }
        ++cases;
        std::vector<float> w((size_t)kh * kw);
        const int sign = below(3);  // mixed, mostly positive, mostly negative
        for (auto& v : w) v = (float)((uniform() - (sign == 0 ? 0.5 : sign == 1 ? 0.1 : 0.9)) / (kh * kw));
        std::vector<double> C((size_t)lm_tbr_const_size(kh, ng));
        lm_tbr_prepare(w.data(), kh, kw, kw, in_x, C.data());
        for (int rep = 0; rep < 4; ++rep) {
          std::vector<uint8_t> M((size_t)kh * ng), m((size_t)kh * ng);
          for (size_t k = 0; k < M.size(); ++k) {
            const int x = below(256), y = rep == 3 ? x : below(256);
            M[k] = (uint8_t)(x > y ? x : y);
            m[k] = (uint8_t)(x > y ? y : x);
          }
          long na = 0, nb = 0;
          std::vector<int> seq_a, seq_b;
          auto ra = [&](int i, int g, unsigned& X, unsigned& n) {
            seq_a.push_back(i * ng + g);
            X = M[(size_t)i * ng + g];
            n = m[(size_t)i * ng + g];
            ++na;
          };
          auto rb = [&](int i, int g, unsigned& X, unsigned& n) {
            seq_b.push_back(i * ng + g);
            X = M[(size_t)i * ng + g];
            n = m[(size_t)i * ng + g];
            ++nb;
          };
          const double S = lm_tbr_sum(kh, ng, C.data(), 0.0, ra);
          std::vector<double> biases = {-1e-3 * (1.0 + uniform()), -S};
          for (int k = 1; k <= 3; ++k) {
            double up = -S, dn = -S;
            for (int s = 0; s < k; ++s) up = std::nextafter(up, INFINITY), dn = std::nextafter(dn, -INFINITY);
            biases.push_back(up);
            biases.push_back(dn);
          }
          for (double bias : biases) {
            seq_a.clear();
            seq_b.clear();
            const double Ua = lm_tbr_sum(kh, ng, C.data(), bias, ra), Ub = lm_tbr_sum_rows(kh, ng, C.data(), bias, rb);
            ++sums;
            neg += Ua < 0.0;
            zero += Ua == 0.0;
            pos += Ua > 0.0;
            if (seq_a != seq_b || (long)seq_a.size() != (long)kh * ng) ++calls;  // the same ranges asked for in the same order
            const bool sn = lm_tbr_sum_negative(kh, ng, C.data(), bias, ra);
            if (!same_bits(Ua, Ub) || sn != (Ub < 0.0)) {
              ++fails;
              printf("FAIL: kh %d kw %d in_x %d bias %.17g: U %.17g against %.17g\n", kh, kw, in_x, bias, Ua, Ub);
            }
          }
        }
      }
  printf("%ld cases, %ld sums, %ld negative, %ld zero, %ld positive, %ld calls differ, %ld failures\n", cases, sums, neg, zero, pos,
         calls, fails);
  return fails || calls ? 1 : 0;
}

struct Det {
  int kh, kw;
  float delta;
  std::vector<float> w;
};
struct View {  // the detector's window inside a view of eh x ew bytes (ew a multiple of 8)
  int eh, ew, in_y, in_x, oh, ow;
};
struct Counts {
  long tiles = 0, refined = 0, kept = 0, ends = 0, middle = 0, proven = 0, shortcol = 0, all = 0, ends_first = 0, sequential = 0,
       fails = 0;
};

// The tiles of one view the tile bound fails (of a point detector: the bright
// ones), their block flags, and the two-round order replayed on them.
void replay_view(const Det& D, const View& G, const uint8_t* ext, bool point, Counts& T) {
  const int oh = G.oh, ow = G.ow, nbw = G.ew / LM_TB_BLK, rows = oh + D.kh - 1;
  const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H, nbx = (ow + LM_TB_BLK - 1) / LM_TB_BLK;
  const int ng = lm_tbr_groups(G.in_x, D.kw);
  std::vector<double> P(D.kh), N(D.kh), C((size_t)lm_tbr_const_size(D.kh, ng));
  double bias = 0;
  if (!lm_tb_prepare(D.w.data(), D.kh, D.kw, D.kw, D.delta, P.data(), N.data(), &bias)) return;
  lm_tbr_prepare(D.w.data(), D.kh, D.kw, D.kw, G.in_x, C.data());
  std::vector<uint8_t> bmax((size_t)G.eh * nbw), bmin((size_t)G.eh * nbw);
  for (int r = 0; r < G.eh; ++r)
    for (int b = 0; b < nbw; ++b)
      lm_tb_row_range(ext + (size_t)r * G.ew, LM_TB_BLK * b, LM_TB_BLK * (b + 1), &bmax[(size_t)r * nbw + b],
                      &bmin[(size_t)r * nbw + b]);
  std::vector<uint8_t> rmax((size_t)rows * ftx), rmin((size_t)rows * ftx);
  for (int r = 0; r < rows; ++r)
    for (int tx = 0; tx < ftx; ++tx) {
      int c0, c1, b0, b1;
      lm_tb_span(tx, D.kw, ow, &c0, &c1);
      lm_tb_blocks(G.in_x, c0, c1, &b0, &b1);
      unsigned mx = 0u, mn = 255u;
      for (int b = b0; b < b1; ++b) {
        const unsigned x = bmax[(size_t)(G.in_y + r) * nbw + b], n = bmin[(size_t)(G.in_y + r) * nbw + b];
        mx = x > mx ? x : mx;
        mn = n < mn ? n : mn;
      }
      rmax[(size_t)r * ftx + tx] = (uint8_t)mx;
      rmin[(size_t)r * ftx + tx] = (uint8_t)mn;
    }
  const uint8_t* win = ext + (size_t)G.in_y * G.ew + G.in_x;
  const int ay = D.kh / 2, ax = D.kw / 2;
  for (int ty = 0; ty < fty; ++ty)
    for (int tx = 0; tx < ftx; ++tx) {
      const int y0 = ty * LM_TB_H, y1 = oh < y0 + LM_TB_H ? oh : y0 + LM_TB_H;
      const int x1 = ow < (tx + 1) * LM_TB_W ? ow : (tx + 1) * LM_TB_W;
      ++T.tiles;
      bool bright = !point;
      for (int y = y0; y < y1 && !bright; ++y)
        for (int x = tx * LM_TB_W; x < x1; ++x) bright |= win[(size_t)(y + ay) * G.ew + x + ax] > 25;
      if (!bright) continue;
      if (lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, D.kh, ty, tx, P.data(), N.data(), bias)) continue;
      ++T.refined;
      const int nb = nbx - tx * LM_TB_NBX < LM_TB_NBX ? nbx - tx * LM_TB_NBX : LM_TB_NBX;
      T.shortcol += nb < LM_TB_NBX;
      bool fl[LM_TB_NBX] = {};
      int first = -1;
      for (int j = 0; j < nb; ++j) {
        fl[j] = !lm_tbr_block_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, ow, D.kh, D.kw, y0, y1 - y0,
                                   tx * LM_TB_NBX + j, C.data(), bias);
        if (fl[j] && first < 0) first = j;
      }
      // the two rounds: an item's block through round_block, a tile's second round only while it is unmarked
      int seen[LM_TB_NBX] = {};
      bool marked = false, by_end = false;
      long summed = 0;
      for (int rd = 0; rd < 2; ++rd) {
        const bool open = !marked;
        for (int q = 0; q < round_items(rd); ++q) {
          const int j = round_block(rd, q, nb);
          if (j < 0 || j > nb) {
            ++T.fails;
            printf("FAIL: round %d item %d of %d blocks is block %d\n", rd, q, nb, j);
            continue;
          }
          if (j == nb) continue;
          ++seen[j];
          if (rd == 1 && !open) continue;
          ++summed;
          if (fl[j]) marked = true, by_end = by_end || rd == 0;
        }
      }
      for (int j = 0; j < nb; ++j)
        if (seen[j] != 1) {
          ++T.fails;
          printf("FAIL: block %d of %d is the item of %d rounds\n", j, nb, seen[j]);
        }
      const bool keep = !lm_tbr_tile_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, oh, ow, D.kh, D.kw, ty, tx, C.data(),
                                          bias, LM_TB_H, false);
      if (marked != keep || keep != (first >= 0)) {
        ++T.fails;
        printf("FAIL: tile (%d, %d) of %d blocks: marked %d, the tile rule keeps %d\n", ty, tx, nb, (int)marked, (int)keep);
      }
      T.kept += keep;
      T.ends += keep && by_end;
      T.middle += keep && !by_end;
      T.proven += !keep;
      T.all += nb;
      T.ends_first += summed;
      T.sequential += keep ? first + 1 : nb;
    }
}

std::vector<float> make_weights(int kind, int kh, int kw) {
  std::vector<double> w((size_t)kh * kw);
  double mean = 0;
  for (int i = 0; i < kh; ++i)
    for (int j = 0; j < kw; ++j) {
      const double y = i - (kh - 1) / 2.0, x = j - (kw - 1) / 2.0;
      const double v = kind == 0 ? (std::fabs(y) <= 1.0 ? 1.0 : -0.35) + 0.02 * (uniform() - 0.5)
                                 : std::exp(-(y * y + x * x) / 6.0) - 0.4 * std::exp(-(y * y + x * x) / 40.0);
      w[(size_t)i * kw + j] = v;
      mean += v;
    }
  mean /= (double)w.size();
  std::vector<float> f(w.size());
  for (size_t k = 0; k < w.size(); ++k) f[k] = (float)((w[k] - mean) / (double)(kh * kw));
  return f;
}

int run_rounds() {
  Counts T;
  // ow % 40 of 8, 16, 24, 32 and 0 (last tile columns of 1 .. 5 blocks), and widths that are no multiple of 8
  const int ows[] = {88, 96, 104, 112, 120, 85, 99, 43, 124, 81, 8, 16, 5};
  const int kws[] = {9, 16, 22, 30, 36, 47};
  int c = 0;
  for (int ow : ows)
    for (int kw : kws)
      for (int kind = 0; kind < 2; ++kind, ++c) {
        Det D;
        D.kw = kw;
        D.kh = 3 + c % 5;
        D.w = make_weights(kind, D.kh, D.kw);
        double sabs = 0;
        for (float v : D.w) sabs += std::fabs((double)v);
        View G;
        G.oh = 9 + c % 4;  // oh % 4 of 1, 2, 3, 0
        G.ow = ow;
        G.in_y = c % 3;
        G.in_x = c % 8 + 8 * (c % 2);
        G.eh = G.in_y + G.oh + D.kh;
        G.ew = (G.in_x + G.ow + D.kw - 1 + LM_TB_BLK - 1) / LM_TB_BLK * LM_TB_BLK;
        for (int im = 0; im < 6; ++im) {
          // bright blobs of several sizes on a dark, slightly noisy ground: a tile's unproven blocks then lie at an
          // end, in the middle or nowhere
          std::vector<uint8_t> img((size_t)G.eh * G.ew);
          const int nblob = 1 + im % 3;
          std::vector<double> cy(nblob), cx(nblob), sg(nblob);
          for (int b = 0; b < nblob; ++b) {
            cy[b] = G.in_y + uniform() * (G.oh + D.kh);
            cx[b] = G.in_x + uniform() * (G.ow + D.kw);
            sg[b] = 1.0 + 5.0 * uniform();
          }
          for (int r = 0; r < G.eh; ++r)
            for (int x = 0; x < G.ew; ++x) {
              double q = 0;
              for (int b = 0; b < nblob; ++b)
                q += std::exp(-((r - cy[b]) * (r - cy[b]) + (x - cx[b]) * (x - cx[b])) / (2.0 * sg[b] * sg[b]));
              img[(size_t)r * G.ew + x] = (uint8_t)(4.0 * uniform() + 240.0 * (q > 1.0 ? 1.0 : q));
            }
          for (double rho : {0.02, 0.08}) {
            D.delta = (float)(-rho * 255.0 * sabs);
            replay_view(D, G, img.data(), false, T);
          }
        }
      }
  printf("%ld tiles, %ld kept by an end, %ld kept by a middle block only, %ld proven, %ld short columns, %ld failures\n", T.refined,
         T.ends, T.middle, T.proven, T.shortcol, T.fails);
  return T.fails ? 1 : 0;
}

int run_views(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    printf("cannot open %s\n", path);
    return 2;
  }
  auto rd = [&](void* p, size_t n) { return fread(p, 1, n, f) == n; };
  auto bad = [&]() {
    fclose(f);
    printf("malformed file\n");
    return 2;
  };
  int32_t ndet = 0;
  if (!rd(&ndet, 4) || ndet < 0 || ndet > 64) return bad();
  long fails = 0;
  Counts A;
  for (int d = 0; d < ndet; ++d) {
    int32_t h[10];  // kh, kw, oh, ow, frames, eh, ew, in_y, in_x, kind (0 point, 1 tail)
    Det D;
    if (!rd(h, sizeof h) || !rd(&D.delta, 4)) return bad();
    D.kh = h[0];
    D.kw = h[1];
    const View G{h[5], h[6], h[7], h[8], h[2], h[3]};
    const int nf = h[4];
    if (D.kh <= 0 || D.kw <= 0 || G.oh <= 0 || G.ow <= 0 || nf < 0 || D.kh > 4096 || D.kw > 4096 || G.oh > 8192 ||
        G.ow > 8192 || G.in_y < 0 || G.in_x < 0 || G.eh > 16384 || G.ew > 16384 || G.ew % LM_TB_BLK != 0 ||
        G.in_y + G.oh + D.kh - 1 > G.eh || G.in_x + G.ow + D.kw - 1 > G.ew)
      return bad();
    D.w.resize((size_t)D.kh * D.kw);
    if (!rd(D.w.data(), D.w.size() * 4)) return bad();
    Counts T;
    std::vector<uint8_t> ext((size_t)G.eh * G.ew);
    for (int k = 0; k < nf; ++k) {
      if (!rd(ext.data(), ext.size())) return bad();
      replay_view(D, G, ext.data(), h[9] == 0, T);
    }
    printf("det %d: refined %ld kept %ld ends %ld all %ld ends_first %ld sequential %ld short %ld failures %ld\n", d, T.refined,
           T.kept, T.ends, T.all, T.ends_first, T.sequential, T.shortcol, T.fails);
    fails += T.fails;
    A.all += T.all;
    A.ends_first += T.ends_first;
    A.sequential += T.sequential;
  }
  fclose(f);
  printf("total: all %ld ends_first %ld sequential %ld\n", A.all, A.ends_first, A.sequential);
  return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "sums") return run_sums();
  if (argc >= 2 && std::string(argv[1]) == "rounds") return run_rounds();
  if (argc >= 3 && std::string(argv[1]) == "views") return run_views(argv[2]);
  printf("usage: tile_sum_rows_check sums | rounds | views FILE\n");
  return 2;
}
