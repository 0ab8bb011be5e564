// narrow_class_check.cpp — the narrow class of ring work items
// (csrc/lm_corr_narrow.h) on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_narrow_class.py.
//
//   narrow_class_check masks
//     every block mask of tiles of 1 .. 5 blocks (last tile columns, ow not a
//     multiple of 8), tried and untried: the class against a brute-force
//     statement of the rule, the item inside its tile, its origin a multiple
//     of 4, the owned columns exactly the unproven blocks' clipped to ow (so
//     the items of a row of tiles cover every unproven block once), and the
//     narrow directory replayed for every wave of many grids.  Prints
//       masks <n> narrow <a> wide <w> grids <g> waves <v> failures <f>
//   narrow_class_check synth
//     synthetic detectors and images as tile_refine_check's: the mask of every
//     tile equals lm_tbr_block_skip block by block, and is empty exactly when
//     lm_tbr_tile_skip proves the tile.  Prints
//       synth <cases> cases tiles <t> kept <k> narrow <a> failures <f>
//   narrow_class_check crops FILE
//     the same on recorded views (tile_refine_check's file format), of the
//     tiles the correlation keeps (bright, proven neither by the tile bound nor
//     by the refinement), and per detector the table
//       det <d>: kept <k> blocks <b> unproven <u> by-count <c1> <c2> <c3> <c4> <c5> span2 <s> untried <t> macs <m> narrow-macs <n> failures <f>
//     (span2: tiles that are narrow; macs: kept tiles x taps x 160 outputs,
//     narrow-macs: the same with narrow tiles at 80 outputs).
//   narrow_class_check entries FILE
//     the same file; per kept tile one line
//       e <det> <frame> <tile> <narrow> <first> <count>
//     (tile: its row-major number on the detector's 40 x 4 grid; first and
//     count 0 for a wide one): what k_tile_bound must list, entry by entry
//     (tests/test_gpu_corr_narrow.py compares the batch's lists with it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_tail_bound.h"
#include "lm_corr_narrow.h"

namespace {

long g_fails = 0;
int g_print_det = -1, g_print_frame = 0;  // entries mode: the detector and frame being listed
#define EXPECT(c, ...)           \
  do {                           \
    if (!(c)) {                  \
      if (g_fails++ < 20) {      \
        printf("FAIL: " __VA_ARGS__); \
        printf("\n");            \
      }                          \
    }                            \
  } while (0)

// ---- masks
// the rule, stated without the header: narrow when tried and last - first < 2
void brute_class(uint32_t m, bool tried, int* narrow, int* first, int* count) {
  int f = -1, l = -1;
  for (int b = 0; b < 5; ++b)
    if (m >> b & 1u) {
      if (f < 0) f = b;
      l = b;
    }
  *narrow = tried && f >= 0 && l - f <= 1;
  *first = f;
  *count = l - f + 1;
}

void run_masks_geometry(long* nmask, long* nnarrow, long* nwide) {
  for (int nb = 1; nb <= 5; ++nb)
    for (int rem = 1; rem <= 8; ++rem)
      for (int tx = 0; tx < 2; ++tx) {
        // tile tx is the last tile column, of nb blocks, the last of them rem columns wide
        const int tile_x = 40 * tx, ow = tile_x + 8 * (nb - 1) + rem;
        for (uint32_t m = 1; m < (1u << nb); ++m)
          for (int tried = 0; tried < 2; ++tried) {
            const uint32_t mask = lm_nw_mask_of(nb, tried != 0, [&](int b) { return (m >> b & 1u) != 0; });
            EXPECT((mask & 31u) == m && ((mask & LM_NW_UNTRIED) != 0u) == (tried == 0), "mask_of(%d, %d, %u) = %u", nb, tried, m, mask);
            const LmNwClass c = lm_nw_classify(mask);
            int bn, bf, bc;
            brute_class(m, tried != 0, &bn, &bf, &bc);
            ++*nmask;
            EXPECT(c.narrow == bn, "mask %u tried %d: class %d, expected %d", m, tried, c.narrow, bn);
            // columns of the tile's unproven blocks, inside ow
            int cover[40] = {0};
            if (!c.narrow) {
              ++*nwide;
              continue;  // (a wide tile runs as the whole tile, as before)
            }
            ++*nnarrow;
            EXPECT(c.first == bf && c.count == bc && c.count >= 1 && c.count <= 2, "mask %u: span %d + %d, expected %d + %d", m,
                   c.first, c.count, bf, bc);
            const int o = lm_nw_origin(c.first);
            EXPECT(o % 4 == 0 && o >= 0 && o + LM_NW_FW <= LM_FW, "first %d: origin %d leaves the tile", c.first, o);
            int x0, x1;
            lm_nw_owned(tile_x, c.first, c.count, ow, &x0, &x1);
            EXPECT(x0 >= tile_x + o && x1 <= tile_x + o + LM_NW_FW, "mask %u: owned [%d, %d) outside the item at %d", m, x0, x1,
                   tile_x + o);
            EXPECT(x1 <= ow && x0 < x1, "mask %u: owned [%d, %d) outside ow %d", m, x0, x1, ow);
            for (int x = x0; x < x1 && x - tile_x < 40 && x >= tile_x; ++x) ++cover[x - tile_x];
            for (int x = 0; x < 40; ++x) {
              const int want = tile_x + x < ow && (m >> (x / 8) & 1u) ? 1 : 0;
              EXPECT(cover[x] == want, "mask %u nb %d ow %d: column %d owned %d times, expected %d", m, nb, ow, tile_x + x,
                     cover[x], want);
            }
            // the entry carries the span
            const uint64_t e = lm_nw_entry(0x01230045u, c.first, c.count);
            EXPECT(lm_nw_entry_tile(e) == 0x01230045u && lm_nw_entry_first(e) == c.first && lm_nw_entry_count(e) == c.count,
                   "entry round trip");
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

// the narrow directory: every wave of a grid finds its detector, segment and items; the waves tile every segment's
// entries in order, and the waves past the total find nothing
void run_directory(long* ngrids, long* nwaves) {
  for (int grid = 0; grid < 400; ++grid) {
    const int n = 1 + grid % LM_NDET;
    std::vector<int32_t> cnt((size_t)n * LM_TL_NC);
    const int style = grid % 5;  // empty, sparse with gaps, dense, multiples of 16, one segment
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < LM_TL_NC; ++c) {
        int v = 0;
        if (style == 1) v = uniform() < 0.2 ? (int)(uniform() * 70) : 0;
        if (style == 2) v = (int)(uniform() * 200);
        if (style == 3) v = 16 * (int)(uniform() * 4);
        if (style == 4) v = c == (grid / 5) % LM_TL_NC ? 1 + (int)(uniform() * 40) : 0;
        if (k == grid % 3 && grid % 7 == 0) v = 0;  // a detector without narrow tiles among others
        cnt[(size_t)k * LM_TL_NC + c] = v;
      }
    int32_t waves[LM_NDET] = {0};
    for (int k = 0; k < n; ++k) waves[k] = lm_nw_listed_waves(&cnt[(size_t)k * LM_TL_NC]);
    const LmCorrDirRecN rec = lm_nw_record(waves, n);
    int total = 0;
    for (int k = 0; k < n; ++k) total += waves[k];
    EXPECT(rec.total == total, "grid %d: total %d, expected %d", grid, rec.total, total);
    std::vector<int> seen((size_t)n * LM_TL_NC, 0);  // entries of each segment handed out so far
    int pk = 0;
    for (int g = 0; g < total + 9; ++g) {
      int k = -1, local = -1;
      const bool ok = lm_nw_lookup(rec, n, g, &k, &local);
      EXPECT(ok == (g < total), "grid %d wave %d: lookup %d past %d", grid, g, (int)ok, total);
      if (!ok) continue;
      ++*nwaves;
      EXPECT(k >= pk && k < n && local >= 0 && local < waves[k], "grid %d wave %d: detector %d wave %d", grid, g, k, local);
      if (k < 0 || k >= n) continue;
      pk = k;
      int c = -1, w = -1, nv = -1;
      const bool found = lm_nw_segment(&cnt[(size_t)k * LM_TL_NC], local, &c, &w, &nv);
      EXPECT(found && c >= 0 && c < LM_TL_NC && nv >= 1 && nv <= LM_NW_NQ, "grid %d wave %d: segment %d items %d", grid, g, c, nv);
      if (!found || c < 0 || c >= LM_TL_NC) continue;
      int& s = seen[(size_t)k * LM_TL_NC + c];
      EXPECT(s == LM_NW_NQ * w, "grid %d wave %d: segment %d place %d, %d entries handed out", grid, g, c, w, s);
      s += nv;
    }
    for (size_t i = 0; i < seen.size(); ++i) EXPECT(seen[i] == cnt[i], "grid %d: counter %zu: %d of %d entries", grid, i, seen[i], cnt[i]);
    ++*ngrids;
  }
  // the grid a launch is given holds the waves of any lists of whole slots
  for (int nt = 1; nt < 40; nt += 3)
    for (int ns = 1; ns < 70; ns += 4) {
      // the worst case: every segment one slot over a multiple of two slots' tiles, every place listed narrow
      int w = 0, left = ns;
      for (int c = 0; c < LM_TL_NC && left > 0; ++c) {
        const int k = (left + (LM_TL_NC - c) - 1) / (LM_TL_NC - c);
        w += lm_nw_seg_waves(8 * nt * k);
        left -= k;
      }
      EXPECT(w <= lm_nw_grid_waves(nt, ns, 1), "grid of %d tiles x %d slots: %d waves in a grid of %d", nt, ns, w,
             lm_nw_grid_waves(nt, ns, 1));
    }
}

int run_masks() {
  long nmask = 0, nnarrow = 0, nwide = 0, ngrids = 0, nwaves = 0;
  run_masks_geometry(&nmask, &nnarrow, &nwide);
  run_directory(&ngrids, &nwaves);
  printf("masks %ld narrow %ld wide %ld grids %ld waves %ld failures %ld\n", nmask, nnarrow, nwide, ngrids, nwaves, g_fails);
  return g_fails ? 1 : 0;
}

// ---- views
struct Det {
  int kh, kw;
  float delta;
  std::vector<float> w;
};
struct View {
  int eh, ew, in_y, in_x, oh, ow;
};
struct Tally {
  long tiles = 0, kept = 0, blocks = 0, unproven = 0, by[6] = {0}, narrow = 0, untried = 0;
};

void check_view(const Det& D, const View& G, const uint8_t* ext, bool point, Tally& T) {
  const int oh = G.oh, ow = G.ow, nbw = G.ew / LM_TB_BLK, rows = oh + D.kh - 1;
  const int ftx = (ow + LM_TB_W - 1) / LM_TB_W, fty = (oh + LM_TB_H - 1) / LM_TB_H;
  const int nbx = (ow + LM_TB_BLK - 1) / LM_TB_BLK;
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
      const int nb = (nbx - tx * LM_TB_NBX < LM_TB_NBX ? nbx - tx * LM_TB_NBX : LM_TB_NBX), nr = y1 - y0;
      const uint32_t mask = lm_nw_mask_of(nb, nr == LM_TB_H, [&](int b) {
        return !lm_tbr_block_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, ow, D.kh, D.kw, y0, nr, tx * LM_TB_NBX + b,
                                  C.data(), bias);
      });
      // block by block against the refinement itself, and as a whole against the tile rule
      int cnt = 0;
      for (int b = 0; b < LM_TB_NBX; ++b) {
        const bool unp = b < nb && !lm_tbr_block_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, ow, D.kh, D.kw, y0, nr,
                                                      tx * LM_TB_NBX + b, C.data(), bias);
        EXPECT(((mask >> b & 1u) != 0) == unp, "tile (%d, %d) block %d: mask bit %u, block_skip %d", ty, tx, b, mask >> b & 1u, !unp);
        cnt += unp;
      }
      const bool proven = lm_tbr_tile_skip(bmax.data(), bmin.data(), nbw, G.in_y, G.in_x, oh, ow, D.kh, D.kw, ty, tx, C.data(),
                                           bias, LM_TB_H, false);
      EXPECT(proven == ((mask & 31u) == 0u), "tile (%d, %d): mask %u but the tile rule says %d", ty, tx, mask, (int)proven);
      if (proven) continue;
      ++T.kept;
      T.blocks += nb;
      T.unproven += cnt;
      ++T.by[cnt];
      const LmNwClass c = lm_nw_classify(mask);
      if (g_print_det >= 0)
        printf("e %d %d %d %d %d %d\n", g_print_det, g_print_frame, ty * ftx + tx, c.narrow, c.narrow ? c.first : 0,
               c.narrow ? c.count : 0);
      T.untried += (mask & LM_NW_UNTRIED) != 0u;
      if (c.narrow) {
        ++T.narrow;
        int o0, o1;
        lm_nw_owned(tx * LM_TB_W, c.first, c.count, ow, &o0, &o1);
        const int org = tx * LM_TB_W + lm_nw_origin(c.first);
        EXPECT(org % 4 == 0 && o0 >= org && o1 <= org + LM_NW_FW && o1 <= ow && org + LM_NW_FW <= (tx + 1) * LM_TB_W,
               "tile (%d, %d): item at %d owns [%d, %d)", ty, tx, org, o0, o1);
        for (int b = 0; b < nb; ++b) {
          const int bx0 = tx * LM_TB_W + 8 * b, bx1 = bx0 + 8 < ow ? bx0 + 8 : ow;
          if (mask >> b & 1u) EXPECT(o0 <= bx0 && bx1 <= o1, "tile (%d, %d): unproven block %d not owned", ty, tx, b);
        }
      }
    }
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
        default: v = uniform() - 0.5; break;                                                            // random sign
      }
      w[(size_t)i * kw + j] = v;
    }
  if (kind < 2) {
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
  long cases = 0;
  const int kws[] = {9, 11, 16, 17, 23, 24, 31, 33, 40, 47, 56, 65, 70};
  const int khs[] = {3, 5, 6, 4};
  const int shapes[][2] = {{9, 85}, {10, 43}, {7, 124}, {6, 81}};  // oh % 4: 1, 2, 3, 2; ow % 8 and ow % 40 != 0
  int c = 0;
  for (int kind = 0; kind < 3; ++kind)
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
      G.in_x = (c * 3 + kind) % 8 + 8 * (c % 2);
      const int rows = G.oh + D.kh - 1, wcols = G.ow + D.kw - 1;
      G.eh = G.in_y + rows + 1;
      G.ew = (G.in_x + wcols + LM_TB_BLK - 1) / LM_TB_BLK * LM_TB_BLK;
      std::vector<std::vector<uint8_t>> imgs;
      auto filled = [&](int v) { return std::vector<uint8_t>((size_t)G.eh * G.ew, (uint8_t)v); };
      for (int e : {0, 3, 9, 22}) {  // vertical steps at several offsets, both orders
        auto im = filled(0);
        for (int r = 0; r < G.eh; ++r)
          for (int x = 0; x < G.ew; ++x) im[(size_t)r * G.ew + x] = (uint8_t)(((x >= G.in_x + 30 + e) != ((e & 1) != 0)) ? 210 : 8);
        imgs.push_back(im);
      }
      for (int b = 0; b < 3; ++b) {  // blobs on a dark, slightly noisy ground
        auto im = filled(0);
        const double cy = G.in_y + 2.0 + 5.0 * uniform(), cx = G.in_x + 20.0 + uniform() * (wcols - 40.0), s = 2.0 + 4.0 * b;
        for (int r = 0; r < G.eh; ++r)
          for (int x = 0; x < G.ew; ++x) {
            const double q = std::exp(-((r - cy) * (r - cy) + (x - cx) * (x - cx)) / (2.0 * s * s));
            im[(size_t)r * G.ew + x] = (uint8_t)(4.0 * uniform() + 240.0 * q);
          }
        imgs.push_back(im);
      }
      {
        auto im = filled(0);
        for (auto& p : im) p = (uint8_t)(uniform() * 255);
        imgs.push_back(im);
      }
      for (double rho : {0.04 * 255.0 * sabs, 0.2 * 255.0 * sabs}) {
        D.delta = (float)(-rho);
        for (const auto& im : imgs) {
          check_view(D, G, im.data(), false, T);
          ++cases;
        }
      }
    }
  printf("synth %ld cases tiles %ld kept %ld narrow %ld failures %ld\n", cases, T.tiles, T.kept, T.narrow, g_fails);
  return g_fails ? 1 : 0;
}

int run_crops(const char* path, bool entries) {
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
    const long before = g_fails;
    for (int k = 0; k < nf; ++k) {
      if (!rd(ext.data(), ext.size()) || !rd(ref.data(), ref.size() * 4)) return bad();
      if (entries) {
        g_print_det = d;
        g_print_frame = k;
      }
      check_view(D, G, ext.data(), h[9] == 0, T);
    }
    const long taps = (long)D.kh * D.kw;
    printf("det %d: kept %ld blocks %ld unproven %ld by-count %ld %ld %ld %ld %ld span2 %ld untried %ld macs %ld narrow-macs %ld failures %ld\n",
           d, T.kept, T.blocks, T.unproven, T.by[1], T.by[2], T.by[3], T.by[4], T.by[5], T.narrow, T.untried,
           T.kept * taps * 160, (T.kept - T.narrow) * taps * 160 + T.narrow * taps * 80, g_fails - before);
  }
  fclose(f);
  return g_fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "masks") return run_masks();
  if (argc >= 2 && std::string(argv[1]) == "synth") return run_synth();
  if (argc >= 3 && std::string(argv[1]) == "crops") return run_crops(argv[2], false);
  if (argc >= 3 && std::string(argv[1]) == "entries") return run_crops(argv[2], true);
  printf("usage: narrow_class_check masks | synth | crops FILE | entries FILE\n");
  return 2;
}
