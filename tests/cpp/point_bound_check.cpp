// point_bound_check.cpp — csrc/lm_tail_bound.h applied to the point detectors
// (paw, snout) on the host (a plain program, also built with
// -fsanitize=address,undefined by tests/test_point_bound.py); the sibling of
// tail_bound_check.cpp.
//
//   point_bound_check crops FILE
//     detectors with recorded windows and the reference's raw scores (written
//     by the test from the oracle's run).  A point score is kept only when it
//     is > 0 and its mouse pixel -- the window pixel under the detector's
//     anchor tap (kh / 2, kw / 2) -- is > 25; a 40 x 4 tile is bright when
//     one of its outputs' mouse pixels is.  For every bright tile: the fused
//     fp32 chain (fmaf per tap) must reproduce the reference's scores bit for
//     bit (the windows are the reference's), and when the predicate says
//     "skip" no output of the tile may be > 0 in the fused chain nor in the
//     unfused one (rounded product, rounded sum), whatever its mouse pixel.
//     Dark tiles are never evaluated by the library and are only counted.
//     Prints per detector
//       det <d>: tiles <t> bright <b> nokept <k> proven <s> mismatch <m> failures <f>
//     (nokept: bright tiles without a kept score; proven: bright tiles skipped).
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
  long tiles = 0, bright = 0, nokept = 0, proven = 0, mismatch = 0, fails = 0;
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

void check_image(const Det& D, const uint8_t* win, int oh, int ow, const float* ref, Tally& T) {
  const int wcols = ow + D.kw - 1, rows = oh + D.kh - 1;
  const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H;
  std::vector<double> P(D.kh), N(D.kh);
  double bias = 0;
  const int on = lm_tb_prepare(D.w.data(), D.kh, D.kw, D.kw, D.delta, P.data(), N.data(), &bias);
  std::vector<uint8_t> rmax((size_t)rows * ftx), rmin((size_t)rows * ftx);
  for (int r = 0; r < rows; ++r)
    for (int tx = 0; tx < ftx; ++tx) {
      int c0, c1;
      lm_tb_span(tx, D.kw, ow, &c0, &c1);
      lm_tb_row_range(win + (size_t)r * wcols, c0, c1, &rmax[(size_t)r * ftx + tx], &rmin[(size_t)r * ftx + tx]);
    }
  const int ay = D.kh / 2, ax = D.kw / 2;  // the anchor tap: output (y, x)'s mouse pixel is window (y + ay, x + ax)
  for (int ty = 0; ty < fty; ++ty)
    for (int tx = 0; tx < ftx; ++tx) {
      const int y1 = oh < (ty + 1) * LM_TB_H ? oh : (ty + 1) * LM_TB_H;
      const int x1 = ow < (tx + 1) * LM_TB_W ? ow : (tx + 1) * LM_TB_W;
      ++T.tiles;
      bool bright = false;
      for (int y = ty * LM_TB_H; y < y1; ++y)
        for (int x = tx * LM_TB_W; x < x1; ++x) bright |= win[(size_t)(y + ay) * wcols + x + ax] > 25;
      if (!bright) continue;
      ++T.bright;
      const bool skip = on && lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, D.kh, ty, tx, P.data(), N.data(), bias);
      bool anypos = false, kept = false;
      for (int y = ty * LM_TB_H; y < y1; ++y)
        for (int x = tx * LM_TB_W; x < x1; ++x) {
          const float f = chain_fused(D, win, wcols, y, x), u = chain_unfused(D, win, wcols, y, x);
          if (memcmp(&f, &ref[(size_t)y * ow + x], 4) != 0) ++T.mismatch;
          if (f > 0.0f || u > 0.0f) {
            anypos = true;
            if (win[(size_t)(y + ay) * wcols + x + ax] > 25) kept = true;
          }
        }
      T.nokept += !kept;
      T.proven += skip;
      if (skip && anypos) {
        ++T.fails;
        printf("FAIL: tile (%d, %d) skipped but holds a positive score (kh %d kw %d delta %.9g)\n", ty, tx, D.kh, D.kw,
               (double)D.delta);
      }
    }
}

int run_crops(const char* path) {
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
  if (!rd(&ndet, 4)) return bad();
  long fails = 0;
  for (int d = 0; d < ndet; ++d) {
    int32_t h[5];
    Det D;
    if (!rd(h, sizeof h) || !rd(&D.delta, 4)) return bad();
    D.kh = h[0];
    D.kw = h[1];
    const int oh = h[2], ow = h[3], nf = h[4];
    if (D.kh <= 0 || D.kw <= 0 || oh <= 0 || ow <= 0 || nf < 0 || D.kh > 4096 || D.kw > 4096 || oh > 8192 || ow > 8192)
      return bad();
    D.w.resize((size_t)D.kh * D.kw);
    if (!rd(D.w.data(), D.w.size() * 4)) return bad();
    Tally T;
    std::vector<uint8_t> win((size_t)(oh + D.kh - 1) * (ow + D.kw - 1));
    std::vector<float> ref((size_t)oh * ow);
    for (int k = 0; k < nf; ++k) {
      if (!rd(win.data(), win.size()) || !rd(ref.data(), ref.size() * 4)) return bad();
      check_image(D, win.data(), oh, ow, ref.data(), T);
    }
    printf("det %d: tiles %ld bright %ld nokept %ld proven %ld mismatch %ld failures %ld\n", d, T.tiles, T.bright,
           T.nokept, T.proven, T.mismatch, T.fails);
    fails += T.fails + T.mismatch;
  }
  fclose(f);
  return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && std::string(argv[1]) == "crops") return run_crops(argv[2]);
  printf("usage: point_bound_check crops FILE\n");
  return 2;
}
