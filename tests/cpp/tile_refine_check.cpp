// tile_refine_check.cpp — the refinement of csrc/lm_tail_bound.h (the bound per
// 8-column output block and group of 8 taps, for the tiles the tile bound
// fails) on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_tile_refine.py.  A detector's
// window lies at (in_y, in_x) of a view (the ext crop on the GPU), and the
// ranges are taken over the view's aligned blocks of 8 columns, as the kernels
// take them.
//
//   tile_refine_check synth
//     detectors (line, DoG, random sign, all positive, all negative) of widths
//     9 .. 70 x every in_x mod 8 x output sizes with ow % 8, ow % 40 and
//     oh % 4 != 0 x images (steps, blobs, noise).  Prints
//       <n> cases, <f> failures, <t> tiles, <b> base, <s> skipped, <p> non-positive, <x> shortcut
//   tile_refine_check crops FILE
//     detectors with recorded views and the reference's raw scores (written by
//     the test from the oracle's run).  Prints "level <LM_TB_RH>", then per detector
//       det <d>: tiles <t> bright <b> nokept <k> base <s0> rh4 <s4> rh1 <s1> shipped <s> mismatch <m> shortcut <x> failures <f>
//
// For every tile (of a point detector: every bright tile, one with a mouse
// pixel > 25 under the anchor tap (kh / 2, kw / 2) of one of its outputs) the
// tile rule is evaluated at block heights 1 and 4 -- base: tiles the tile
// bound proves alone; rh4 / rh1: with the refinement; shipped: at LM_TB_RH --
// and no skipped tile may hold a positive score in the fused fp32 chain (fmaf
// per tap) nor in the unfused one.  shortcut counts the tiles whose flag at
// height 1 differs between the evaluation with the four-row shortcut and
// without it, and a tile proven at height 4 but not at height 1 is a failure.
// With reference scores the fused chain must reproduce them bit for bit.
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

struct View {  // the detector's window inside a view of eh x ew bytes (ew a multiple of 8)
  int eh, ew, in_y, in_x, oh, ow;
};

struct Tally {
  long cases = 0, tiles = 0, bright = 0, nokept = 0, base = 0, rh4 = 0, rh1 = 0, shipped = 0, mismatch = 0, shortcut = 0,
       fails = 0, positive = 0;
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

// One view: the tile rule of every (bright) tile against both chains.  `ref`:
// the reference's scores (oh x ow) or null; `point`: only bright tiles count.
void check_view(const Det& D, const View& G, const uint8_t* ext, const float* ref, bool point, bool expect_never, Tally& T) {
  const int oh = G.oh, ow = G.ow, nbw = G.ew / LM_TB_BLK, rows = oh + D.kh - 1;
  const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H;
  const int ng = lm_tbr_groups(G.in_x, D.kw);
  std::vector<double> P(D.kh), N(D.kh), C((size_t)lm_tbr_const_size(D.kh, ng));
  double bias = 0;
  const int on = lm_tb_prepare(D.w.data(), D.kh, D.kw, D.kw, D.delta, P.data(), N.data(), &bias);
  lm_tbr_prepare(D.w.data(), D.kh, D.kw, D.kw, G.in_x, C.data());
  ++T.cases;
  if (expect_never && on) {
    ++T.fails;
    printf("FAIL: a detector that must never skip was accepted (delta %g)\n", (double)D.delta);
  }
  {  // the groups partition the taps
    int next = 0;
    for (int g = 0; g < ng; ++g) {
      int j0, j1;
      lm_tbr_taps(G.in_x, D.kw, g, &j0, &j1);
      if (j0 != next || j1 <= j0 || j1 - j0 > LM_TB_BLK || (G.in_x + j0) / LM_TB_BLK != (G.in_x + j1 - 1) / LM_TB_BLK) {
        ++T.fails;
        printf("FAIL: tap group %d of %d is [%d, %d) (in_x %d kw %d)\n", g, ng, j0, j1, G.in_x, D.kw);
        return;
      }
      next = j1;
    }
    if (next != D.kw) {
      ++T.fails;
      printf("FAIL: the tap groups end at %d of %d taps\n", next, D.kw);
      return;
    }
  }
  // the view's block ranges, then the tile bound's row ranges from them (as k_tile_bound_ref takes them)
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
  const uint8_t* win = ext + (size_t)G.in_y * G.ew + G.in_x;  // the window, pitch ew
  const int ay = D.kh / 2, ax = D.kw / 2;
  for (int ty = 0; ty < fty; ++ty)
    for (int tx = 0; tx < ftx; ++tx) {
      const int y1 = oh < (ty + 1) * LM_TB_H ? oh : (ty + 1) * LM_TB_H;
      const int x1 = ow < (tx + 1) * LM_TB_W ? ow : (tx + 1) * LM_TB_W;
      ++T.tiles;
      bool bright = !point;
      for (int y = ty * LM_TB_H; y < y1 && !bright; ++y)
        for (int x = tx * LM_TB_W; x < x1; ++x) bright |= win[(size_t)(y + ay) * G.ew + x + ax] > 25;
      if (!bright) continue;
      ++T.bright;
      auto refined = [&](int rh, bool shortcut) {
        return lm_tbr_tile_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, oh, ow, D.kh, D.kw, ty, tx, C.data(), bias,
                                rh, shortcut);
      };
      const bool base = on && lm_tb_tile_skip(rmax.data(), rmin.data(), ftx, oh, D.kh, ty, tx, P.data(), N.data(), bias);
      const bool s4 = base || (on && refined(LM_TB_H, false));
      const bool s1 = base || (on && refined(1, false));
      const bool s1s = base || (on && refined(1, true));
      const bool shipped = LM_TB_RH == 1 ? s1s : s4;
      bool anypos = false, kept = false;
      for (int y = ty * LM_TB_H; y < y1; ++y)
        for (int x = tx * LM_TB_W; x < x1; ++x) {
          const float f = chain_fused(D, win, G.ew, y, x), u = chain_unfused(D, win, G.ew, y, x);
          if (ref && memcmp(&f, &ref[(size_t)y * ow + x], 4) != 0) ++T.mismatch;
          if (f > 0.0f || u > 0.0f) {
            anypos = true;
            if (!point || win[(size_t)(y + ay) * G.ew + x + ax] > 25) kept = true;
          }
        }
      T.nokept += !kept;
      T.positive += anypos;
      T.base += base;
      T.rh4 += s4;
      T.rh1 += s1;
      T.shipped += shipped;
      T.shortcut += s1 != s1s;
      if (s4 && !s1) {
        ++T.fails;
        printf("FAIL: tile (%d, %d) proven over four rows but not row by row\n", ty, tx);
      }
      if ((s1 || s4 || s1s) && anypos) {
        ++T.fails;
        printf("FAIL: tile (%d, %d) skipped but holds a positive score (kh %d kw %d in_x %d delta %.9g)\n", ty, tx, D.kh,
               D.kw, G.in_x, (double)D.delta);
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
        case 0: v = (std::fabs(y) <= 1.0 ? 1.0 : -0.35) + 0.02 * (uniform() - 0.5); break;              // line
        case 1: v = std::exp(-(y * y + x * x) / 6.0) - 0.4 * std::exp(-(y * y + x * x) / 40.0); break;  // DoG
        case 2: v = uniform() - 0.5; break;                                                             // random sign
        case 3: v = 0.1 + uniform(); break;                                                             // all positive
        default: v = -0.1 - uniform(); break;                                                           // all negative
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

int run_synth() {
  Tally T;
  const int kws[] = {9, 11, 16, 17, 23, 24, 31, 33, 40, 47, 56, 65, 70};
  const int khs[] = {3, 5, 6, 4};
  const int shapes[][2] = {{9, 85}, {10, 43}, {7, 124}, {6, 81}};  // oh % 4: 1, 2, 3, 2; ow % 8 and ow % 40 != 0
  int c = 0;
  for (int kind = 0; kind < 5; ++kind)
    for (int kwi = 0; kwi < 13; ++kwi, ++c) {
      Det D;
      D.kw = kws[kwi];
      D.kh = khs[c % 4];
      D.w = make_weights(kind, D.kh, D.kw);
      double sabs = 0;
      for (float v : D.w) sabs += std::fabs((double)v);
      View G;
      G.oh = shapes[c % 4][0];
      G.ow = shapes[c % 4][1];
      G.in_y = c % 3;
      G.in_x = (c * 3 + kind) % 8 + 8 * (c % 2);  // (3 c + kind) mod 8 runs through every residue
      const int rows = G.oh + D.kh - 1, wcols = G.ow + D.kw - 1;
      G.eh = G.in_y + rows + 1;
      G.ew = (G.in_x + wcols + LM_TB_BLK - 1) / LM_TB_BLK * LM_TB_BLK;
      std::vector<std::vector<uint8_t>> imgs;
      auto filled = [&](int v) { return std::vector<uint8_t>((size_t)G.eh * G.ew, (uint8_t)v); };
      imgs.push_back(filled(0));
      imgs.push_back(filled(255));
      for (int e : {0, 3, 9, 22}) {  // vertical steps at several offsets, both orders
        auto im = filled(0);
        for (int r = 0; r < G.eh; ++r)
          for (int x = 0; x < G.ew; ++x) im[(size_t)r * G.ew + x] = (uint8_t)(((x >= G.in_x + 30 + e) != ((e & 1) != 0)) ? 210 : 8);
        imgs.push_back(im);
      }
      for (int e : {1, 2}) {  // horizontal steps
        auto im = filled(0);
        for (int r = 0; r < G.eh; ++r)
          for (int x = 0; x < G.ew; ++x) im[(size_t)r * G.ew + x] = (uint8_t)(((r >= G.in_y + 4 + e) != (e == 2)) ? 200 : 10);
        imgs.push_back(im);
      }
      for (int b = 0; b < 2; ++b) {  // blobs on a dark, slightly noisy ground
        auto im = filled(0);
        const double cy = G.in_y + 2.0 + 5.0 * uniform(), cx = G.in_x + 20.0 + uniform() * (wcols - 40.0), s = 2.0 + 9.0 * b;
        for (int r = 0; r < G.eh; ++r)
          for (int x = 0; x < G.ew; ++x) {
            const double q = std::exp(-((r - cy) * (r - cy) + (x - cx) * (x - cx)) / (2.0 * s * s));
            im[(size_t)r * G.ew + x] = (uint8_t)(4.0 * uniform() + 240.0 * q);
          }
        imgs.push_back(im);
      }
      for (int amp : {3, 255}) {  // noise
        auto im = filled(0);
        for (auto& p : im) p = (uint8_t)(uniform() * amp);
        imgs.push_back(im);
      }
      const double rhos[3] = {0.04 * 255.0 * sabs, 0.2 * 255.0 * sabs, 0.0};
      for (int ri = 0; ri < 3; ++ri) {
        D.delta = (float)(-rhos[ri]);
        for (size_t k = (ri == 2 ? 8 : 0); k < imgs.size(); ++k)
          check_view(D, G, imgs[k].data(), nullptr, false, !(D.delta < 0.0f), T);
      }
    }
  {  // non-finite weights: never skipped
    Det D;
    D.kh = 3;
    D.kw = 12;
    D.delta = -5.0f;
    View G{12, 104, 1, 5, 9, 85};
    for (float bad : {NAN, INFINITY, -INFINITY}) {
      D.w.assign(36, -0.01f);
      D.w[17] = bad;
      std::vector<uint8_t> im((size_t)G.eh * G.ew, 0);
      check_view(D, G, im.data(), nullptr, false, true, T);
    }
  }
  printf("%ld cases, %ld failures, %ld tiles, %ld base, %ld skipped, %ld non-positive, %ld shortcut\n", T.cases, T.fails,
         T.tiles, T.base, T.shipped, T.tiles - T.positive, T.shortcut);
  return T.fails || T.shortcut ? 1 : 0;
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
  printf("level %d\n", LM_TB_RH);  // the shipped block height
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
    Tally T;
    std::vector<uint8_t> ext((size_t)G.eh * G.ew);
    std::vector<float> ref((size_t)G.oh * G.ow);
    for (int k = 0; k < nf; ++k) {
      if (!rd(ext.data(), ext.size()) || !rd(ref.data(), ref.size() * 4)) return bad();
      check_view(D, G, ext.data(), ref.data(), h[9] == 0, false, T);
    }
    printf("det %d: tiles %ld bright %ld nokept %ld base %ld rh4 %ld rh1 %ld shipped %ld mismatch %ld shortcut %ld failures %ld\n",
           d, T.tiles, T.bright, T.nokept, T.base, T.rh4, T.rh1, T.shipped, T.mismatch, T.shortcut, T.fails);
    fails += T.fails + T.mismatch + T.shortcut;
  }
  fclose(f);
  return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "synth") return run_synth();
  if (argc >= 3 && std::string(argv[1]) == "crops") return run_crops(argv[2]);
  printf("usage: tile_refine_check synth | crops FILE\n");
  return 2;
}
