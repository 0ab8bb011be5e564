/*
 * lm_tile_plan.h — the host's plan of the tile-bound pre-pass (plain C++: the
 * host runtime and tests/cpp/tile_plan_check.cpp share it; no HIP call, no
 * environment): the tail tile grids, the bound's and the refinement's
 * constants per detector (lm_tail_bound.h), k_tile_bound_ref's LDS and
 * k_tile_bound's bands and LDS (LmConst::tt_*, pt_plane, tb_*, tbr_*, tbw_*).
 * The kernels trust these fields without a check; this file is their
 * definition, and tests/cpp/tile_plan_check.cpp asserts on the CPU what
 * k_tile_bound relies on.
 *
 * k_tile_bound's LDS for one band of view v, all byte offsets (lm_tbw_layout
 * lays it out, LmTbwLayout holds it, LmConst::tbw_* is its copy):
 *   0           block ranges B: u16 max | min << 8 per ext row and block of
 *               the columns tbw_blo .. + tbw_nbk (both even: a 32-bit word
 *               holds two blocks), tbw_rows rows: the most a band loads;
 *   tbw_v       their four-row windows V, tbw_rows - 3 rows; when a detector
 *               of the view is refined they become their pair table in place
 *               (entry b: the range over blocks b and b + 1), and a spare row
 *               and 16 bytes follow, since a term's three words are fetched a
 *               chunk ahead without a clamp: behind the last chunk of the last
 *               weight row they are the row below's;
 *   tbw_al      (refined views) per detector k the windows' entries at the
 *               last block of its window, u16, at k * tbw_rows: tbw_rows - 3
 *               rows are written, one more is fetched ahead;
 *   tbw_pn[d]   (8-aligned) per used detector P_i then N_i, 2 kh doubles;
 *   tbw_win[d]  per used detector the window table: wmax, then wmin at
 *               + tbw_wsz[d]; tbw_wsz[d]: the entries of its largest band;
 *   tbw_ent[d]  (4-aligned) per listed detector the band's list entries, one
 *               word per tile of tbw_br tile rows;
 *   tbw_work    the tiles to evaluate, one word per tile of the band over the
 *               listed detectors; later the marks of the refined entries;
 *   tbw_lds[v]  bytes in all, at most kTbwLds.
 */
#ifndef LM_TILE_PLAN_H
#define LM_TILE_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "lm_device.h"
#include "lm_tail_bound.h"

// k_ingest: each thread owns 16 consecutive crop bytes of its band, and writes
// their block ranges (two blocks) as one word for k_tile_bound
#define LM_INGEST_VEC 16
static_assert(LM_FW >= LM_INGEST_VEC, "a 16-byte chunk spans at most two flag tiles");
static_assert(LM_TB_BLK == 8 && LM_INGEST_VEC == 2 * LM_TB_BLK, "a 16-byte chunk holds two blocks");
#define LM_INGEST_MAXTX 128  // flag-grid columns a band's workgroup can hold (ow <= 128 LM_FW)

static_assert(LM_TB_W == LM_FW && LM_TB_H == LM_FH, "the bound's tiles are the dark-tile grid's");
#define LM_TB_THREADS 256
#ifndef LM_TBW_TILES
#define LM_TBW_TILES LM_TB_THREADS  // k_tile_bound: about this many tiles of a view's detectors per band
#endif
#ifndef LM_TBW_ROW_LOOP
#define LM_TBW_ROW_LOOP 1  // 1 = k_tile_bound<true> (lm_tbr_sum_rows_n) where all refined detectors allow it; 0 = lm_tbr_sum for all
#endif

constexpr int64_t kTbRefLds = 144 * 1024;  // k_tile_bound_ref's LDS, per view
constexpr int64_t kTbwLds = 64 * 1024;     // k_tile_bound's, per band

// What the context asks for, before the plan's own force-offs.
struct LmTileSwitches {
  bool tailskip;   // skip the tail detectors' proven tiles (LM_CORR_TAILSKIP)
  bool pointskip;  // the same for the point detectors' bright tiles (LM_CORR_POINTSKIP)
  bool refine;     // refine the tiles the tile bound fails (LM_TILE_REFINE)
  bool f16;        // the f16 correlation: the bound is for the fp32 chain, both skips off
  bool dark;       // dark tiles (LM_CORR_DARK): the point skip starts from k_ingest's bright flags, off without them
  bool screen = true;  // the refinement's fp32 screen ahead of the double sum (LM_TILE_SCREEN)
};

struct LmTilePlan {
  std::vector<double> tbc;  // the bound constants: per detector P_i, N_i at tb_off, the group constants at tbr_off
  size_t tb_lds = 0;        // k_tile_bound_ref's LDS bytes (the larger view's)
  size_t tbw_lds = 0;       // k_tile_bound's (the larger view's band)
  bool row_loop = false;    // the pre-pass is k_tile_bound<true> (a used, refined detector of one chunk per weight row)
  bool tailskip = false, pointskip = false;  // the switches after every force-off
};

// A view's three detectors (ids 3 v + k) on k_tile_bound's bands.
struct LmTbwView {
  int v;
  int ftx[3], ty[3];  // tile columns and rows of detector k's grid
  bool on[3];         // its tiles are listed by the pre-pass
  int sum_tx;         // tile columns over the listed detectors
  int br, nband;      // tile rows per band, bands
};

// The LDS of a band of a view for the set `use` of detectors with a bound
// (the layout at the top; the LmConst::tbw_* fields of the same names).
struct LmTbwLayout {
  int32_t blo, nbk, rows, v, al, work;
  int32_t use[3], pn[3], win[3], wsz[3], ent[3];
  uint32_t inv[3];
  int64_t lds;
};

// The tail tile grids, the point detectors' flag planes, and the limits of a
// list entry (slot << 16 | tile), which switch a skip off.
// Reads det[], fl_tx, fl_ty, fl_slot; fills tt_*, pt_plane.
inline void lm_tp_grids(LmConst& K, int nslots, bool* tailskip, bool* pointskip) {
  int o = 0, mt = 0;
  for (int t = 0; t < 2; ++t) {
    const LmDet& D = K.det[t ? DET_TAIL_S : DET_TAIL_B];
    K.tt_tx[t] = (D.ow + LM_FW - 1) / LM_FW;
    K.tt_ty[t] = (D.oh + LM_FH - 1) / LM_FH;
    K.tt_off[t] = o;
    o += (K.tt_tx[t] * K.tt_ty[t] + 3) / 4 * 4;
    mt = std::max(mt, K.tt_tx[t] * K.tt_ty[t]);
  }
  K.tt_slot = o;
  K.tt_stride = nslots * mt;
  if (mt > 65535 || nslots > 65535) *tailskip = false;
  // the point detectors' own flags: k_ingest's layout once per feature (lists: tl_stride each)
  static_assert(LIST_PAW_B == 0 && LIST_SNOUT_B == 1 && LIST_PAW_S == 2 && LIST_SNOUT_S == 3, "list l: feature l & 1");
  K.pt_plane = (int64_t)K.fl_slot * nslots;
  if (K.fl_tx[0] * K.fl_ty[0] > 65535 || K.fl_tx[1] * K.fl_ty[1] > 65535 || nslots > 65535) *pointskip = false;
}

// The bound's constants per detector of view v, appended to tbc (from the
// fp32 weights the kernels use), and k_tile_bound_ref's LDS: the view's block
// ranges, then the row ranges of each detector whose bound is usable and fits
// (the tail detector first).  Reads det[], ext_h, ext_w, fl_tx, tt_tx; fills
// tb_off, tb_skip, tb_bias, tb_rng, tb_lds[v], tbr_on, tbr_ng, tbr_off, tbs_*.
inline void lm_tp_bounds(LmConst& K, int v, const float* wts, bool tailskip, bool pointskip, bool refine, bool screen,
                         std::vector<double>& tbc) {
  int64_t lds = 2 * (int64_t)K.ext_h[v] * (K.ext_w[v] / LM_TB_BLK);
  bool any = false;
  for (int d : {3 * v + 2, 3 * v, 3 * v + 1}) {
    const LmDet& D = K.det[d];
    K.tb_off[d] = (int32_t)tbc.size();
    tbc.resize(tbc.size() + 2 * (size_t)D.kh);
    K.tb_skip[d] = lm_tb_prepare(wts + D.w_off, D.kh, D.kw, D.kwp, D.delta, tbc.data() + K.tb_off[d],
                                 tbc.data() + K.tb_off[d] + D.kh, &K.tb_bias[d]);
    const int64_t rows = (int64_t)D.oh + D.kh - 1, wcols = (int64_t)D.ow + D.kw - 1;
    const int64_t need = 2 * rows * (D.kind != 0 ? K.tt_tx[v] : K.fl_tx[v]);
    const bool inside = D.in_y >= 0 && D.in_x >= 0 && D.in_y + rows <= K.ext_h[v] && D.in_x + wcols <= K.ext_w[v];
    if (!(D.kind != 0 ? tailskip : pointskip) || !inside || lds + need > kTbRefLds) K.tb_skip[d] = 0;
    K.tb_rng[d] = K.tb_skip[d] ? (int32_t)lds : 0;
    if (K.tb_skip[d]) {
      lds += need;
      any = true;
    }
    // the refinement's constants per tap group (off wherever the skip is)
    K.tbr_on[d] = K.tb_skip[d] && refine ? 1 : 0;
    K.tbr_ng[d] = K.tbr_on[d] ? lm_tbr_groups(D.in_x, D.kw) : 0;
    tbc.resize((tbc.size() + 7) / 8 * 8);  // (a chunk of group constants is 64 bytes, kept aligned)
    K.tbr_off[d] = (int32_t)tbc.size();
    if (K.tbr_on[d]) {
      tbc.resize(tbc.size() + (size_t)lm_tbr_const_size(D.kh, K.tbr_ng[d]));
      lm_tbr_prepare(wts + D.w_off, D.kh, D.kw, D.kwp, D.in_x, tbc.data() + K.tbr_off[d]);
    }
    // the screen's constants: floats, kept among the doubles (a row is 32 bytes, kept aligned)
    K.tbs_on[d] = 0;
    K.tbs_off[d] = (int32_t)tbc.size();
    K.tbs_bf[d] = K.tbs_e[d] = 0.f;
    if (K.tbr_on[d] && screen && lm_tbr_chunks(K.tbr_ng[d]) == 1) {
      static_assert(LM_TBS_ROW * sizeof(float) == 4 * sizeof(double), "a row of the screen's floats is four doubles");
      std::vector<float> cf((size_t)D.kh * LM_TBS_ROW);
      const LmTbsConst R = lm_tbs_prepare(tbc.data() + K.tbr_off[d], D.kh, K.tbr_ng[d], K.tb_bias[d], 1, cf.data());
      tbc.resize(tbc.size() + cf.size() / 2);
      std::memcpy(tbc.data() + K.tbs_off[d], cf.data(), cf.size() * sizeof(float));
      K.tbs_on[d] = R.on;
      K.tbs_bf[d] = R.bf;
      K.tbs_e[d] = R.E;
    }
  }
  K.tb_lds[v] = any ? (int32_t)lds : 0;
}

// k_tile_bound's bands of view v: tile rows per band so that the band's tiles
// over the view's listed detectors are about one workgroup's threads, evenly
// over the bands.  Reads det[], fl_tx, fl_ty, tt_tx, tt_ty.
inline LmTbwView lm_tbw_view(const LmConst& K, int v, bool tailskip, bool pointskip) {
  LmTbwView W{};
  W.v = v;
  int max_ty = 1;
  for (int k = 0; k < 3; ++k) {
    const LmDet& D = K.det[3 * v + k];
    W.ftx[k] = D.kind != 0 ? K.tt_tx[v] : K.fl_tx[v];
    W.ty[k] = D.kind != 0 ? K.tt_ty[v] : K.fl_ty[v];
    W.on[k] = D.kind != 0 ? tailskip : pointskip;
    if (W.on[k]) {
      W.sum_tx += W.ftx[k];
      max_ty = std::max(max_ty, W.ty[k]);
    }
  }
  const int br0 = std::max(1, LM_TBW_TILES / std::max(1, W.sum_tx));
  const int nband = (max_ty + br0 - 1) / br0;
  W.br = (max_ty + nband - 1) / nband;
  W.nband = (max_ty + W.br - 1) / W.br;
  return W;
}

// The most ext rows a band of the view loads, for the set `use` of detectors
// with a bound (the kernel's y_lo .. y_hi).  Reads det[], ext_h.
inline int lm_tbw_band_rows(const LmConst& K, const LmTbwView& W, const bool (&use)[3]) {
  const int v = W.v;
  int rows = 0;
  for (int j = 0; j < W.nband; ++j) {
    int y_lo = K.ext_h[v], y_hi = 0;
    for (int k = 0; k < 3; ++k) {
      const LmDet& D = K.det[3 * v + k];
      int t0, nty;
      const int ohb = lm_tbw_band(D, W.ty[k], W.br, j, &t0, &nty);
      if (!use[k] || nty == 0) continue;
      y_lo = std::min(y_lo, D.in_y + LM_FH * t0);
      y_hi = std::max(y_hi, D.in_y + LM_FH * t0 + ohb + D.kh - 1);
    }
    rows = std::max(rows, std::min(y_hi, K.ext_h[v]) - y_lo);
  }
  return rows;
}

// The band's LDS for the set `use`.  Reads det[], ext_h, ext_w, tbr_on.
inline LmTbwLayout lm_tbw_layout(const LmConst& K, const LmTbwView& W, const bool (&use)[3]) {
  const int v = W.v;
  LmTbwLayout L{};
  int b_lo = K.ext_w[v] / LM_TB_BLK, b_hi = 0;
  for (int k = 0; k < 3; ++k) {
    const LmDet& D = K.det[3 * v + k];
    if (!use[k]) continue;
    b_lo = std::min(b_lo, D.in_x / LM_TB_BLK);
    b_hi = std::max(b_hi, (D.in_x + D.ow + D.kw - 1 + LM_TB_BLK - 1) / LM_TB_BLK);
  }
  b_lo = b_lo / 2 * 2;
  b_hi = std::min((b_hi + 1) / 2 * 2, K.ext_w[v] / LM_TB_BLK);
  L.blo = b_lo < b_hi ? b_lo : 0;
  L.nbk = b_lo < b_hi ? b_hi - b_lo : 0;
  L.rows = std::max(0, lm_tbw_band_rows(K, W, use));
  int64_t o = 2 * (int64_t)L.rows * L.nbk;
  L.v = (int32_t)o;
  o += 2 * (int64_t)std::max(0, L.rows - (LM_TB_H - 1)) * L.nbk;
  // when a detector of the view is refined, the windows become their pair table (lm_tbr_pair_word) in place:
  // a spare row and three words behind them (a term's words are fetched a chunk ahead, without a clamp), and
  // per detector the windows' entries at the last block of its window (rows entries each: one spare)
  bool pairs = false;
  for (int k = 0; k < 3; ++k) pairs = pairs || (use[k] && K.tbr_on[3 * v + k] != 0);
  if (pairs) o += 2 * (int64_t)L.nbk + 16;
  L.al = (int32_t)o;
  if (pairs) o += 2 * 3 * (int64_t)L.rows;
  o = (o + 7) / 8 * 8;
  for (int k = 0; k < 3; ++k) {
    const LmDet& D = K.det[3 * v + k];
    L.use[k] = use[k] ? 1 : 0;
    L.inv[k] = lm_rcp(W.ftx[k]);
    L.pn[k] = (int32_t)o;
    if (use[k]) o += 16 * (int64_t)D.kh;
  }
  for (int k = 0; k < 3; ++k) {
    const LmDet& D = K.det[3 * v + k];
    int wsz = 0;
    for (int j = 0; use[k] && j < W.nband; ++j) {
      int t0, nty;
      const int ohb = lm_tbw_band(D, W.ty[k], W.br, j, &t0, &nty);
      if (nty) wsz = std::max(wsz, lm_tb_win_rows(ohb, D.kh) * W.ftx[k]);
    }
    L.win[k] = (int32_t)o;
    L.wsz[k] = wsz;
    o += 2 * (int64_t)wsz;
  }
  o = (o + 3) / 4 * 4;
  for (int k = 0; k < 3; ++k) {
    L.ent[k] = (int32_t)o;
    if (W.on[k]) o += 4 * (int64_t)W.br * W.ftx[k];
  }
  L.work = (int32_t)o;
  o += 4 * (int64_t)W.br * W.sum_tx;
  L.lds = o;
  return L;
}

// k_tile_bound's bands and LDS of view v: every listed detector with a bound
// (and at most LM_TB_THREADS / 2 weight rows: a thread loads one of its P_i,
// N_i), less the detectors that have to lose theirs for the band to fit
// kTbwLds: the snout's, the paw's, the tail's, in that order (the tail
// detector is the last to lose its bound, as in k_tile_bound_ref).
// Reads det[], ext_h, ext_w, fl_*, tt_*, tb_skip, tbr_on; fills tbw_*.
inline void lm_tp_bands(LmConst& K, int v, bool tailskip, bool pointskip) {
  const LmTbwView W = lm_tbw_view(K, v, tailskip, pointskip);
  bool use[3];
  for (int k = 0; k < 3; ++k)
    use[k] = W.on[k] && K.tb_skip[3 * v + k] != 0 && 2 * K.det[3 * v + k].kh <= LM_TB_THREADS;
  LmTbwLayout L = lm_tbw_layout(K, W, use);
  for (int k : {1, 0, 2}) {
    if (L.lds <= kTbwLds) break;
    use[k] = false;
    L = lm_tbw_layout(K, W, use);
  }
  if (L.lds > kTbwLds) throw std::invalid_argument("bounding box too wide for the tile lists' workgroup.");
  K.tbw_br[v] = W.br;
  K.tbw_nband[v] = W.nband;
  K.tbw_blo[v] = L.blo;
  K.tbw_nbk[v] = L.nbk;
  K.tbw_rows[v] = L.rows;
  K.tbw_v[v] = L.v;
  K.tbw_al[v] = L.al;
  K.tbw_work[v] = L.work;
  K.tbw_lds[v] = (int32_t)L.lds;
  for (int k = 0; k < 3; ++k) {
    const int d = 3 * v + k;
    K.tbw_use[d] = L.use[k];
    K.tbw_inv[d] = L.inv[k];
    K.tbw_pn[d] = L.pn[k];
    K.tbw_win[d] = L.win[k];
    K.tbw_wsz[d] = L.wsz[k];
    K.tbw_ent[d] = L.ent[k];
  }
}

// The whole plan.  K holds det[], ext_h, ext_w, fl_tx, fl_ty and fl_slot;
// wts: the fp32 weights, rows zero-padded to kwp, detector d's at det[d].w_off.
// Fills K's tt_*, pt_plane, tb_*, tbr_* and tbw_* and returns the rest.
// Build with -ffp-contract=off, as the library is.
inline LmTilePlan lm_tile_plan(LmConst& K, int nslots, const float* wts, const LmTileSwitches& sw) {
  LmTilePlan R;
  R.tailskip = sw.tailskip;
  R.pointskip = sw.pointskip;
  if (sw.f16) R.tailskip = R.pointskip = false;  // the bound is for the fp32 chain
  if (!sw.dark) R.pointskip = false;             // it starts from k_ingest's bright flags
  lm_tp_grids(K, nslots, &R.tailskip, &R.pointskip);
  for (int v = 0; v < 2; ++v) {
    lm_tp_bounds(K, v, wts, R.tailskip, R.pointskip, sw.refine, sw.screen, R.tbc);
    R.tb_lds = std::max(R.tb_lds, (size_t)K.tb_lds[v]);
  }
  for (int v = 0; v < 2; ++v) {
    lm_tp_bands(K, v, R.tailskip, R.pointskip);
    R.tbw_lds = std::max(R.tbw_lds, (size_t)K.tbw_lds[v]);
  }
  bool one_chunk = false;
  for (int d = 0; d < LM_NDET; ++d)
    one_chunk = one_chunk || (K.tbw_use[d] && K.tbr_on[d] && lm_tbr_chunks(K.tbr_ng[d]) == 1);
  R.row_loop = LM_TBW_ROW_LOOP && one_chunk;
  return R;
}

#endif  // LM_TILE_PLAN_H
