// tail_bound_check.cpp — csrc/lm_tail_bound.h on the host (a plain program,
// also built with -fsanitize=address,undefined by tests/test_tail_bound.py).
//
//   tail_bound_check synth
//     detectors (line, DoG, random sign, all positive, all negative) x rho
//     (positive, zero, negative, tiny) x images (uniform, two-level horizontal
//     and vertical edges at every offset inside a tile, noise), and cases
//     whose rho puts the largest true score within 1e-4 of 0.  Whenever the
//     predicate says "skip", no output of the tile may be > 0 in the fused
//     fp32 chain (fmaf per tap) nor in the unfused one (rounded product,
//     rounded sum).  Prints "<n> cases, <f> failures, <t> tiles, <s> skipped".
//   tail_bound_check crops FILE
//     detectors with recorded windows and the reference's scores (written by
//     the test from the oracle's run): the fused chain must reproduce the
//     scores bit for bit (the windows are the reference's), the predicate must
//     hold, and the share of skipped tiles per detector is printed.
//
// Build with -ffp-contract=off: the unfused chain must stay unfused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_tail_bound.h"

namespace {

struct Det {
  int kh, kw;
  float delta;
  std::vector<float> w;
};

struct Tally {
  long cases = 0, fails = 0, tiles = 0, skipped = 0, nonpos = 0, mismatch = 0;
};

float chain_fused(const Det& D, const uint8_t* win, int pitch, int y, int x) {
  float a = D.delta;
  for (int i = 0; i < D.kh; ++i)
    for (int j = 0; j < D.kw; ++j) a = fmaf(D.w[i * D.kw + j], (float)win[(y + i) * pitch + x + j], a);
  return a;
}

float chain_unfused(const Det& D, const uint8_t* win, int pitch, int y, int x) {
  float a = D.delta;
  for (int i = 0; i < D.kh; ++i)
    for (int j = 0; j < D.kw; ++j) {
      volatile float prod = D.w[i * D.kw + j] * (float)win[(y + i) * pitch + x + j];
      a = a + prod;
    }
  return a;
}

// One image: the predicate of every tile against both chains.  `ref`: the
// reference's scores (oh x ow) to compare the fused chain with, or null.
void check_image(const Det& D, const uint8_t* win, int oh, int ow, const float* ref, Tally& T, bool expect_never) {
  const int wcols = ow + D.kw - 1, rows = oh + D.kh - 1;
  const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H;
  std::vector<double> P(D.kh), N(D.kh);
  double bias = 0;
  const int on = lm_tb_prepare(D.w.data(), D.kh, D.kw, D.kw, D.delta, P.data(), N.data(), &bias);
  ++T.cases;
  if (expect_never && on) {
    ++T.fails;
    printf("FAIL: a detector that must never skip was accepted (delta %g)\n", (double)D.delta);
  }
  std::vector<uint8_t> rmax((size_t)rows * ftx), rmin((size_t)rows * ftx);
  for (int r = 0; r < rows; ++r)
    for (int tx = 0; tx < ftx; ++tx) {
      int c0, c1;
      lm_tb_span(tx, D.kw, ow, &c0, &c1);
      if (c0 < 0 || c1 > wcols || c1 < (tx + 1 == ftx ? wcols : (tx + 1) * LM_TB_W + D.kw - 1)) {
        ++T.fails;
        printf("FAIL: span [%d, %d) of tile column %d does not cover its taps\n", c0, c1, tx);
        return;
      }
      lm_tb_row_range(win + (size_t)r * wcols, c0, c1, &rmax[(size_t)r * ftx + tx], &rmin[(size_t)r * ftx + tx]);
    }
  for (int ty = 0; ty < fty; ++ty)
    for (int tx = 0; tx < ftx; ++tx) {
      const bool skip = on && lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, D.kh, ty, tx, P.data(), N.data(), bias);
      bool anypos = false;
      for (int y = ty * LM_TB_H; y < oh && y < (ty + 1) * LM_TB_H; ++y)
        for (int x = tx * LM_TB_W; x < ow && x < (tx + 1) * LM_TB_W; ++x) {
          const float f = chain_fused(D, win, wcols, y, x), u = chain_unfused(D, win, wcols, y, x);
          if (ref && memcmp(&f, &ref[(size_t)y * ow + x], 4) != 0) ++T.mismatch;
          if (f > 0.0f || u > 0.0f) anypos = true;
        }
      ++T.tiles;
      T.skipped += skip;
      T.nonpos += !anypos;
      if (skip && anypos) {
        ++T.fails;
        printf("FAIL: tile (%d, %d) skipped but holds a positive score (kh %d kw %d delta %.9g)\n", ty, tx, D.kh, D.kw,
               (double)D.delta);
      }
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform() {  // [0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

std::vector<float> make_weights(int kind, int kh, int kw) {
  std::vector<double> w((size_t)kh * kw);
  for (int i = 0; i < kh; ++i)
    for (int j = 0; j < kw; ++j) {
      const double y = i - (kh - 1) / 2.0, x = j - (kw - 1) / 2.0;
      double v;
      switch (kind) {
        case 0: v = (std::fabs(y) <= 1.0 ? 1.0 : -0.35) + 0.02 * (uniform() - 0.5); break;             // line
        case 1: v = std::exp(-(y * y + x * x) / 3.0) - 0.4 * std::exp(-(y * y + x * x) / 12.0); break;  // DoG
        case 2: v = uniform() - 0.5; break;                                                            // random sign
        case 3: v = 0.1 + uniform(); break;                                                            // all positive
        default: v = -0.1 - uniform(); break;                                                          // all negative
      }
      w[(size_t)i * kw + j] = v;
    }
  if (kind < 2) {  // zero mean, like the synthetic detectors
    double m = 0;
    for (double v : w) m += v;
    m /= (double)w.size();
    for (double& v : w) v -= m;
  }
  std::vector<float> f(w.size());
  for (size_t k = 0; k < w.size(); ++k) f[k] = (float)(w[k] / (double)(kh * kw));
  return f;
}

double max_exact_score(const Det& D, const uint8_t* win, int oh, int ow) {  // with delta = 0, in double
  const int wcols = ow + D.kw - 1;
  double best = -1e300;
  for (int y = 0; y < oh; ++y)
    for (int x = 0; x < ow; ++x) {
      double a = 0;
      for (int i = 0; i < D.kh; ++i)
        for (int j = 0; j < D.kw; ++j) a += (double)D.w[i * D.kw + j] * (double)win[(y + i) * wcols + x + j];
      best = a > best ? a : best;
    }
  return best;
}

int run_synth() {
  Tally T;
  const int oh = 9, ow = 85;  // three tile rows (the last of one row), three tile columns (the last of five)
  const int sizes[5][2] = {{6, 9}, {7, 7}, {5, 12}, {3, 5}, {4, 4}};
  for (int kind = 0; kind < 5; ++kind) {
    Det D;
    D.kh = sizes[kind][0];
    D.kw = sizes[kind][1];
    D.w = make_weights(kind, D.kh, D.kw);
    double sabs = 0;
    for (float v : D.w) sabs += std::fabs((double)v);
    const int rows = oh + D.kh - 1, wcols = ow + D.kw - 1;
    std::vector<std::vector<uint8_t>> imgs;
    auto blank = [&](int v) { return std::vector<uint8_t>((size_t)rows * wcols, (uint8_t)v); };
    for (int v : {0, 1, 128, 255}) imgs.push_back(blank(v));
    for (int e = 0; e < LM_TB_H; ++e)  // horizontal edges at every row offset inside a tile, both orders
      for (int o = 0; o < 2; ++o) {
        auto im = blank(0);
        for (int r = 0; r < rows; ++r)
          for (int c = 0; c < wcols; ++c) im[(size_t)r * wcols + c] = (uint8_t)(((r >= LM_TB_H + e) != (o != 0)) ? 200 : 10);
        imgs.push_back(im);
      }
    for (int e = 0; e < LM_TB_W; ++e) {  // vertical edges at every column offset inside a tile
      auto im = blank(0);
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < wcols; ++c) im[(size_t)r * wcols + c] = (uint8_t)(((c >= LM_TB_W + e) != ((e & 1) != 0)) ? 255 : 0);
      imgs.push_back(im);
    }
    for (int amp : {3, 40, 255}) {  // noise around a dark level
      auto im = blank(0);
      for (auto& p : im) p = (uint8_t)(uniform() * amp);
      imgs.push_back(im);
    }
    const double rhos[4] = {0.2 * 255.0 * sabs, 0.0, -0.05 * 255.0 * sabs, 1e-30};
    for (int ri = 0; ri < 4; ++ri) {
      D.delta = (float)(-rhos[ri]);
      for (const auto& im : imgs) check_image(D, im.data(), oh, ow, nullptr, T, !(D.delta < 0.0f));
    }
    // rho chosen so that the largest true score lies within 1e-4 of 0 (both sides)
    for (size_t k = 0; k < imgs.size(); k += 7)
      for (double off : {-1e-4, -1e-6, 0.0, 1e-6, 1e-4}) {
        D.delta = (float)(-(max_exact_score(D, imgs[k].data(), oh, ow) + off));
        check_image(D, imgs[k].data(), oh, ow, nullptr, T, !(D.delta < 0.0f));
      }
  }
  {  // non-finite weights: never skipped, whatever the image
    Det D;
    D.kh = 3;
    D.kw = 4;
    D.delta = -5.0f;
    for (float bad : {NAN, INFINITY, -INFINITY}) {
      D.w.assign(12, -0.01f);
      D.w[5] = bad;
      std::vector<uint8_t> im((size_t)(oh + 2) * (ow + 3), 0);
      check_image(D, im.data(), oh, ow, nullptr, T, true);
    }
  }
  printf("%ld cases, %ld failures, %ld tiles, %ld skipped, %ld non-positive\n", T.cases, T.fails, T.tiles, T.skipped,
         T.nonpos);
  return T.fails ? 1 : 0;
}

int run_crops(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    printf("cannot open %s\n", path);
    return 2;
  }
  auto rd = [&](void* p, size_t n) { return fread(p, 1, n, f) == n; };
  int32_t ndet = 0;
  if (!rd(&ndet, 4)) return 2;
  long fails = 0;
  for (int d = 0; d < ndet; ++d) {
    int32_t h[5];
    Det D;
    if (!rd(h, sizeof h) || !rd(&D.delta, 4)) return 2;
    D.kh = h[0];
    D.kw = h[1];
    const int oh = h[2], ow = h[3], nf = h[4];
    if (D.kh <= 0 || D.kw <= 0 || oh <= 0 || ow <= 0 || nf < 0 || D.kh > 4096 || D.kw > 4096 || oh > 8192 || ow > 8192)
      return 2;
    D.w.resize((size_t)D.kh * D.kw);
    if (!rd(D.w.data(), D.w.size() * 4)) return 2;
    Tally T;
    std::vector<uint8_t> win((size_t)(oh + D.kh - 1) * (ow + D.kw - 1));
    std::vector<float> ref((size_t)oh * ow);
    for (int k = 0; k < nf; ++k) {
      if (!rd(win.data(), win.size()) || !rd(ref.data(), ref.size() * 4)) return 2;
      check_image(D, win.data(), oh, ow, ref.data(), T, false);
    }
    printf("det %d: tiles %ld skipped %ld nonpositive %ld mismatch %ld failures %ld\n", d, T.tiles, T.skipped, T.nonpos,
           T.mismatch, T.fails);
    fails += T.fails + T.mismatch;
  }
  fclose(f);
  return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "synth") return run_synth();
  if (argc >= 3 && std::string(argv[1]) == "crops") return run_crops(argv[2]);
  printf("usage: tail_bound_check synth | crops FILE\n");
  return 2;
}
