// tile_screen_check.cpp — the fp32 screen of the refinement's block sum
// (csrc/lm_tail_bound.h: lm_tbs_*) against the double sum it stands in front
// of (lm_tbr_sum), on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_tile_screen.py.
//
// A "disagreement" is a decided item whose decision is not lm_tbr_sum < 0.
// Every prepared detector's constants are checked as well (const_fails): Pf >=
// P, Nf <= N, bf >= bias, all of them normal or zero, and E at least the
// margin of the header's proof, recomputed here in long double.
//
//   tile_screen_check sums
//     kh 1 .. 40, 1 .. 4 tap groups at every in_x % 8, random weights and byte
//     ranges; biases that put U_d at zero, 1 .. 3 ulps to either side, and at
//     -+E/2 and -+2.5 E.  Every |U_d| >= 2 E must be decided.  Prints
//       <c> cases, <s> sums, <neg> negative, <pos> positive, <u> undecided, <d> disagreements, <b> undecided beyond 2E,
//       <k> const_fails
//   tile_screen_check adversarial
//     Weights that strain the margin or trip the gate.  Prints per set
//       set <name>: screened <0|1> sums <s> undecided <u> disagreements <d> const_fails <k>
//   tile_screen_check views FILE [MASKS]
//     Recorded views (tests/test_tile_sum_rows.py::write_views' format): the
//     blocks of full-height tiles that the refinement sums -- of the tiles the
//     tile bound fails (of a point detector: the bright ones), or, with MASKS
//     (per detector and frame one byte per tile, row-major), of the tiles set
//     there.  Prints per detector
//       det <d>: screened <0|1> items <n> negative <neg> undecided <u> disagreements <x> const_fails <k>
//
// Build with -ffp-contract=off, as the library is built.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_tail_bound.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
double uniform() { return (double)(next64() >> 11) / 9007199254740992.0; }  // [0, 1)
int below(int n) { return (int)(uniform() * n); }

struct Tally {
  long sums = 0, neg = 0, pos = 0, und = 0, dis = 0, beyond = 0, cfail = 0;
};

bool normal_or_zero(float f) { return f == 0.f || std::fabs(f) >= FLT_MIN; }

// The constants of a screened detector against the doubles they stand for and
// the margin against the proof's formula.
long check_constants(const double* C, int kh, int ng, double bias, const float* Cf, const LmTbsConst& R) {
  long bad = 0;
  long double sum = 0;
  for (int i = 0; i < kh; ++i)
    for (int g = 0; g < LM_TBR_GC; ++g) {
      const float pf = Cf[i * LM_TBS_ROW + 2 * g], nf = -Cf[i * LM_TBS_ROW + 2 * g + 1];
      const double p = g < ng ? C[i * 2 * LM_TBR_GC + g] : 0.0, n = g < ng ? C[(i * 2 + 1) * LM_TBR_GC + g] : 0.0;
      if (!((double)pf >= p) || !((double)nf <= n) || nf < 0.f || !normal_or_zero(pf) || !normal_or_zero(nf)) ++bad;
      // (one float ulp at the most)
      if ((double)pf > p * (1.0 + 1.2e-7) || (double)nf < n * (1.0 - 1.2e-7)) ++bad;
      sum += (long double)pf + (long double)nf;
    }
  if (!((double)R.bf >= bias) || !normal_or_zero(R.bf)) ++bad;
  const long double n = (long double)kh * ng, S = std::fabs((long double)R.bf) + 255.0L * sum;
  const long double E = 2.0L * (2.0L * n + 4.0L) * ldexpl(1.0L, -24) * S + (n + 2.0L) * ldexpl(1.0L, -51) * S + (n + 1.0L) * 2.4e-38L;
  if (!((long double)R.E >= E)) ++bad;
  if (bad) printf("FAIL: constants of kh %d ng %d bias %.17g: %ld checks\n", kh, ng, bias, bad);
  return bad;
}

// One item: the screen's decision against the double sum's sign.
template <class F>
void one_sum(int kh, int ng, const double* C, double bias, const float* Cf, const LmTbsConst& R, F&& rng, Tally& T,
             const char* what) {
  const double Ud = lm_tbr_sum(kh, ng, C, bias, rng);
  const float Uf = lm_tbs_sum_rows(kh, ng, Cf, R.bf, rng);
  const int dec = lm_tbs_decide(Uf, R.E);
  ++T.sums;
  T.neg += dec < 0;
  T.pos += dec > 0;
  T.und += dec == 0;
  if ((dec < 0 && !(Ud < 0.0)) || (dec > 0 && Ud < 0.0)) {
    ++T.dis;
    printf("FAIL: %s kh %d ng %d bias %.17g: U_f %.9g E %.9g decides %d, U_d %.17g\n", what, kh, ng, bias, (double)Uf, (double)R.E,
           dec, Ud);
  }
  if (dec == 0 && std::fabs(Ud) >= 2.0 * (double)R.E) {
    ++T.beyond;
    printf("FAIL: %s kh %d ng %d bias %.17g: U_d %.17g undecided beyond 2 E = %.9g\n", what, kh, ng, bias, Ud, 2.0 * (double)R.E);
  }
}

// The items of one detector (its group constants C) over random and extreme
// ranges at biases around the negated sum of the terms.  Returns whether the
// screen took the detector at its own bias.
bool strain(int kh, int ng, const double* C, double own_bias, int ok, int reps, Tally& T, const char* what) {
  std::vector<float> Cf((size_t)kh * LM_TBS_ROW);
  const LmTbsConst R0 = lm_tbs_prepare(C, kh, ng, own_bias, ok, Cf.data());
  if (R0.on) T.cfail += check_constants(C, kh, ng, own_bias, Cf.data(), R0);
  for (int rep = 0; rep < reps; ++rep) {
    std::vector<uint8_t> M((size_t)kh * ng), m((size_t)kh * ng);
    for (size_t k = 0; k < M.size(); ++k) {
      const int x = rep == 0 ? 255 : rep == 1 ? 0 : below(256), y = rep == 0 ? 0 : rep == 1 ? 0 : rep == 2 ? x : below(256);
      M[k] = (uint8_t)(x > y ? x : y);
      m[k] = (uint8_t)(x > y ? y : x);
    }
    auto rng = [&](int i, int g, unsigned& X, unsigned& n) {
      X = M[(size_t)i * ng + g];
      n = m[(size_t)i * ng + g];
    };
    const double S = lm_tbr_sum(kh, ng, C, 0.0, rng);
    const LmTbsConst Rz = lm_tbs_prepare(C, kh, ng, -S, ok, Cf.data());
    const double E = (double)Rz.E;
    std::vector<double> biases = {own_bias, -S, -S - 0.5 * E, -S + 0.5 * E, -S - 2.5 * E, -S + 2.5 * E};
    for (int k = 1; k <= 3; ++k) {
      double up = -S, dn = -S;
      for (int s = 0; s < k; ++s) up = std::nextafter(up, INFINITY), dn = std::nextafter(dn, -INFINITY);
      biases.push_back(up);
      biases.push_back(dn);
    }
    for (double bias : biases) {
      const LmTbsConst R = lm_tbs_prepare(C, kh, ng, bias, ok, Cf.data());
      if (!R.on) continue;
      T.cfail += check_constants(C, kh, ng, bias, Cf.data(), R);
      one_sum(kh, ng, C, bias, Cf.data(), R, rng, T, what);
    }
  }
  return R0.on != 0;
}

int run_sums() {
  Tally T;
  long cases = 0;
  for (int kh = 1; kh <= 40; ++kh)
    for (int ng = 1; ng <= LM_TBR_GC; ++ng)
      for (int a = 0; a < LM_TB_BLK; ++a) {
        const int lo = LM_TB_BLK * (ng - 1) - a + 1 > 1 ? LM_TB_BLK * (ng - 1) - a + 1 : 1, hi = LM_TB_BLK * ng - a;
        if (hi < lo) continue;
        const int kw = lo + below(hi - lo + 1), in_x = a + LM_TB_BLK * below(3);
        if (lm_tbr_groups(in_x, kw) != ng) {
          ++T.dis;
          printf("FAIL: kw %d at in_x %d has %d groups, not %d\n", kw, in_x, lm_tbr_groups(in_x, kw), ng);
          continue;
        }
        ++cases;
        std::vector<float> w((size_t)kh * kw);
        const int sign = below(3);  // mixed, mostly positive, mostly negative
        double sabs = 0;
        for (auto& v : w) {
          v = (float)((uniform() - (sign == 0 ? 0.5 : sign == 1 ? 0.1 : 0.9)) / (kh * kw));
          sabs += std::fabs((double)v);
        }
        std::vector<double> P(kh), N(kh), C((size_t)lm_tbr_const_size(kh, ng));
        double bias = 0;
        const int ok = lm_tb_prepare(w.data(), kh, kw, kw, (float)(-0.05 * 255.0 * sabs), P.data(), N.data(), &bias);
        lm_tbr_prepare(w.data(), kh, kw, kw, in_x, C.data());
        if (!strain(kh, ng, C.data(), bias, ok, 5, T, "sums")) {
          ++T.dis;
          printf("FAIL: kh %d kw %d in_x %d is not screened\n", kh, kw, in_x);
        }
      }
  printf("%ld cases, %ld sums, %ld negative, %ld positive, %ld undecided, %ld disagreements, %ld undecided beyond 2E, %ld const_fails\n",
         cases, T.sums, T.neg, T.pos, T.und, T.dis, T.beyond, T.cfail);
  return T.dis || T.beyond || T.cfail ? 1 : 0;
}

int run_adversarial() {
  struct Set {
    const char* name;
    int kh, kw, in_x;
    float delta;
    std::vector<float> w;
  };
  std::vector<Set> sets;
  auto fill = [](int kh, int kw, auto&& f) {
    std::vector<float> w((size_t)kh * kw);
    for (int i = 0; i < kh; ++i)
      for (int j = 0; j < kw; ++j) w[(size_t)i * kw + j] = f(i, j);
    return w;
  };
  sets.push_back({"one huge tap among tiny ones", 24, 30, 2, -1.0f,
                  fill(24, 30, [](int i, int j) { return i == 11 && j == 13 ? 3.0e7f : (float)(1e-9 * (uniform() - 0.5)); })});
  sets.push_back({"one huge negative tap among tiny ones", 16, 25, 0, -1e-3f,
                  fill(16, 25, [](int i, int j) { return i == 3 && j == 24 ? -8.0e5f : (float)(1e-12 * uniform()); })});
  sets.push_back({"all-positive rows", 30, 30, 2, -40.0f, fill(30, 30, [](int, int) { return (float)(1e-3 * (0.5 + uniform())); })});
  sets.push_back({"all-negative rows", 30, 30, 2, -1e-4f, fill(30, 30, [](int, int) { return (float)(-1e-3 * (0.5 + uniform())); })});
  sets.push_back({"rows of one sign each, alternating", 22, 20, 5, -3.0f,
                  fill(22, 20, [](int i, int) { return (float)((i & 1 ? -1.0 : 1.0) * 1e-3 * (0.5 + uniform())); })});
  sets.push_back({"weights near FLT_MIN", 16, 25, 0, -1e-30f,
                  fill(16, 25, [](int, int j) { return (float)((j & 1 ? -1.0 : 1.0) * FLT_MIN * (1.0 + 3.0 * uniform())); })});
  sets.push_back({"weights below FLT_MIN", 16, 25, 0, -1e-3f,
                  fill(16, 25, [](int i, int j) { return i == 2 && j < 8 ? (j == 3 ? 1e-41f : 0.f) : (float)(1e-3 * (uniform() - 0.5)); })});
  sets.push_back({"a tap group of zeros", 24, 30, 2, -0.5f,
                  fill(24, 30, [](int, int j) { return j >= 6 && j < 14 ? 0.f : (float)(2e-3 * (uniform() - 0.5)); })});
  sets.push_back({"delta near zero", 24, 30, 2, -1e-30f, fill(24, 30, [](int, int) { return (float)(1e-3 * (uniform() - 0.5)); })});
  sets.push_back({"sums beyond the floats", 26, 30, 2, -1.0f, fill(26, 30, [](int, int) { return 1e30f; })});
  long fails = 0;
  for (const Set& s : sets) {
    Tally T;
    const int ng = lm_tbr_groups(s.in_x, s.kw);
    std::vector<double> P(s.kh), N(s.kh), C((size_t)lm_tbr_const_size(s.kh, ng));
    double bias = 0;
    const int ok = lm_tb_prepare(s.w.data(), s.kh, s.kw, s.kw, s.delta, P.data(), N.data(), &bias);
    lm_tbr_prepare(s.w.data(), s.kh, s.kw, s.kw, s.in_x, C.data());
    const bool on = strain(s.kh, ng, C.data(), bias, ok, 40, T, s.name);
    printf("set %s: screened %d sums %ld undecided %ld disagreements %ld const_fails %ld\n", s.name, (int)on, T.sums, T.und, T.dis,
           T.cfail);
    fails += T.dis + T.cfail;
  }
  return fails ? 1 : 0;
}

int run_views(const char* path, const char* masks) {
  FILE* f = fopen(path, "rb");
  FILE* fm = masks ? fopen(masks, "rb") : nullptr;
  if (!f || (masks && !fm)) {
    printf("cannot open %s\n", !f ? path : masks);
    if (f) fclose(f);
    return 2;
  }
  auto rd = [&](void* p, size_t n) { return fread(p, 1, n, f) == n; };
  auto bad = [&]() {
    fclose(f);
    if (fm) fclose(fm);
    printf("malformed file\n");
    return 2;
  };
  int32_t ndet = 0;
  if (!rd(&ndet, 4) || ndet < 0 || ndet > 64) return bad();
  long fails = 0;
  for (int d = 0; d < ndet; ++d) {
    int32_t h[10];  // kh, kw, oh, ow, frames, eh, ew, in_y, in_x, kind (0 point, 1 tail)
    float delta;
    if (!rd(h, sizeof h) || !rd(&delta, 4)) return bad();
    const int kh = h[0], kw = h[1], oh = h[2], ow = h[3], nf = h[4], eh = h[5], ew = h[6], in_y = h[7], in_x = h[8];
    if (kh <= 0 || kw <= 0 || oh <= 0 || ow <= 0 || nf < 0 || kh > 4096 || kw > 4096 || oh > 8192 || ow > 8192 || in_y < 0 ||
        in_x < 0 || eh > 16384 || ew > 16384 || ew % LM_TB_BLK != 0 || in_y + oh + kh - 1 > eh || in_x + ow + kw - 1 > ew)
      return bad();
    std::vector<float> w((size_t)kh * kw);
    if (!rd(w.data(), w.size() * 4)) return bad();
    const int nbw = ew / LM_TB_BLK, rows = oh + kh - 1, ng = lm_tbr_groups(in_x, kw);
    const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H, nbx = (ow + LM_TB_BLK - 1) / LM_TB_BLK;
    std::vector<double> P(kh), N(kh), C((size_t)lm_tbr_const_size(kh, ng));
    std::vector<float> Cf((size_t)kh * LM_TBS_ROW);
    double bias = 0;
    const int ok = lm_tb_prepare(w.data(), kh, kw, kw, delta, P.data(), N.data(), &bias);
    lm_tbr_prepare(w.data(), kh, kw, kw, in_x, C.data());
    LmTbsConst R{0.f, 0.f, 0};
    if (lm_tbr_chunks(ng) == 1) R = lm_tbs_prepare(C.data(), kh, ng, bias, ok, Cf.data());
    Tally T;
    if (R.on) T.cfail += check_constants(C.data(), kh, ng, bias, Cf.data(), R);
    std::vector<uint8_t> ext((size_t)eh * ew), mask((size_t)fty * ftx);
    for (int k = 0; k < nf; ++k) {
      if (!rd(ext.data(), ext.size())) return bad();
      if (fm && fread(mask.data(), 1, mask.size(), fm) != mask.size()) return bad();
      if (!ok || !R.on) continue;
      std::vector<uint8_t> bmax((size_t)eh * nbw), bmin((size_t)eh * nbw);
      for (int r = 0; r < eh; ++r)
        for (int b = 0; b < nbw; ++b)
          lm_tb_row_range(ext.data() + (size_t)r * ew, LM_TB_BLK * b, LM_TB_BLK * (b + 1), &bmax[(size_t)r * nbw + b],
                          &bmin[(size_t)r * nbw + b]);
      std::vector<uint8_t> rmax((size_t)rows * ftx), rmin((size_t)rows * ftx);
      for (int r = 0; r < rows; ++r)
        for (int tx = 0; tx < ftx; ++tx) {
          int c0, c1, b0, b1;
          lm_tb_span(tx, kw, ow, &c0, &c1);
          lm_tb_blocks(in_x, c0, c1, &b0, &b1);
          unsigned mx = 0u, mn = 255u;
          for (int b = b0; b < b1; ++b) {
            const unsigned x = bmax[(size_t)(in_y + r) * nbw + b], n = bmin[(size_t)(in_y + r) * nbw + b];
            mx = x > mx ? x : mx;
            mn = n < mn ? n : mn;
          }
          rmax[(size_t)r * ftx + tx] = (uint8_t)mx;
          rmin[(size_t)r * ftx + tx] = (uint8_t)mn;
        }
      const uint8_t* win = ext.data() + (size_t)in_y * ew + in_x;
      const int ay = kh / 2, ax = kw / 2;
      for (int ty = 0; ty < fty; ++ty)
        for (int tx = 0; tx < ftx; ++tx) {
          const int y0 = ty * LM_TB_H, y1 = oh < y0 + LM_TB_H ? oh : y0 + LM_TB_H;
          if (y1 - y0 != LM_TB_H) continue;  // (a short last tile row is summed in double from the block ranges)
          if (fm) {
            if (!mask[(size_t)ty * ftx + tx]) continue;
          } else {
            const int x1 = ow < (tx + 1) * LM_TB_W ? ow : (tx + 1) * LM_TB_W;
            bool bright = h[9] != 0;
            for (int y = y0; y < y1 && !bright; ++y)
              for (int x = tx * LM_TB_W; x < x1; ++x) bright |= win[(size_t)(y + ay) * ew + x + ax] > 25;
            if (!bright) continue;
            if (lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, kh, ty, tx, P.data(), N.data(), bias)) continue;
          }
          for (int xb = tx * LM_TB_NBX; xb < (tx + 1) * LM_TB_NBX && xb < nbx; ++xb) {
            const bool neg = lm_tbr_block_skip(bmax.data(), bmin.data(), nbw, in_y, in_x, ow, kh, kw, y0, LM_TB_H, xb, C.data(), bias);
            const int dec = lm_tbs_block(bmax.data(), bmin.data(), nbw, in_y, in_x, ow, kh, kw, y0, LM_TB_H, xb, Cf.data(), R.bf, R.E);
            ++T.sums;
            T.neg += neg;
            T.und += dec == 0;
            if ((dec < 0 && !neg) || (dec > 0 && neg)) {
              ++T.dis;
              printf("FAIL: det %d frame %d tile (%d, %d) block %d: decision %d, the double sum is %s\n", d, k, ty, tx, xb, dec,
                     neg ? "negative" : "not negative");
            }
          }
        }
    }
    printf("det %d: screened %d items %ld negative %ld undecided %ld disagreements %ld const_fails %ld\n", d, R.on, T.sums, T.neg,
           T.und, T.dis, T.cfail);
    fails += T.dis + T.cfail;
  }
  fclose(f);
  if (fm) fclose(fm);
  return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "sums") return run_sums();
  if (argc >= 2 && std::string(argv[1]) == "adversarial") return run_adversarial();
  if (argc >= 3 && std::string(argv[1]) == "views") return run_views(argv[2], argc >= 4 ? argv[3] : nullptr);
  printf("usage: tile_screen_check sums | adversarial | views FILE [MASKS]\n");
  return 2;
}
