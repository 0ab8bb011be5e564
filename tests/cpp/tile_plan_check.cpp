// tile_plan_check.cpp — the host's plan of the tile-bound pre-pass
// (csrc/lm_tile_plan.h: the tbw_* / tb_* / tbr_* fields of LmConst, which
// k_tile_bound and k_tile_bound_ref trust without a check) against what the
// kernels read, on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_tile_plan.py.
//
// For a list of geometries it fills LmConst's input fields by hand (det[],
// ext_h, ext_w, fl_tx, fl_ty, fl_slot; no pixels), runs lm_tile_plan and
// walks every view and band the way k_tile_bound does, asserting at each
// address the kernel forms that it lies where the plan put it.  Each check
// names the kernel statement it stands for (lm_kernels.hip, k_tile_bound
// unless k_tile_bound_ref is named).
//
// Prints
//   <g> geometries, <v> views, <b> bands, <l> lost, <r> rowloop, <n> generic, <u> unrefined, <x> residues,
//   rem <a> <b> <c>, lastcol <d> <e>, tall <t>, onerow <o>, low <w>, w9 <p> w70 <q>, oddblk <s>, keep101 <i> keep001 <j>,
//   off <k>, nobound <m>, <c> checks, <f> failures
// (lost: detectors that lost their bound to the 64 KB; rowloop / generic /
// unrefined: views with a used, refined detector of one chunk per weight row,
// with refined detectors of more chunks only, without a refined detector;
// residues: values of in_x mod 8 among the used detectors; rem: used detectors
// whose last tile row has 1, 2, 3 output rows; lastcol: whose last tile column
// has one, two output blocks; tall: taller than a band's output rows; low:
// views lower than one band of tile rows; oddblk: views whose windows start in
// an odd block; keep101 / keep001: views that kept
// paw and tail / the tail alone; off: plans with a skip switched off; nobound:
// detectors with delta >= 0.)
//
// Build with -ffp-contract=off, as the library is.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lm_tile_plan.h"

namespace {

struct Tally {
  long geoms = 0, views = 0, bands = 0, lost = 0, rowloop = 0, generic = 0, unrefined = 0;
  unsigned residues = 0;
  long rem[4] = {0, 0, 0, 0}, lastcol[3] = {0, 0, 0}, tall = 0, onerow = 0, low = 0, w9 = 0, w70 = 0;
  long oddblk = 0, keep101 = 0, keep001 = 0, off = 0, nobound = 0, checks = 0, fails = 0;
};
Tally T;
std::string g_where;

void check(bool ok, const char* what, long a = 0, long b = 0) {
  ++T.checks;
  if (!ok && T.fails++ < 20) std::printf("FAIL %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
}

// One view's point-detector output region and its detectors (paw, snout, tail: rows x cols).
struct ViewSpec {
  int oh, ow;
  int kh[3], kw[3];
};
struct Geom {
  const char* name;
  ViewSpec view[2];
  int xshift = 0;      // extra columns left of every window (in_x mod 8)
  bool tight = false;  // the ext crop ends with the lowest window row (else with the correlation tiles' rows)
  int nslots = 9;
  LmTileSwitches sw = {true, true, true, false, true};
  float delta[LM_NDET] = {-6.f, -3.5f, -20.f, -5.f, -5.5f, -22.f};
};

int ceil_half(int v) { return (v + 1) / 2; }

// LmConst's inputs of the plan, as the runtime's steps before it fill them
// (fill_detectors, fill_flag_grid); returns the floats of the padded weights.
int fill_inputs(LmConst& K, const Geom& G) {
  std::memset(&K, 0, sizeof(K));
  const int tw = std::max(1, (int)(G.view[0].ow * 0.6));  // tail_sub_bounding_box 0.6 of the bottom box
  int w_off = 0;
  for (int v = 0; v < 2; ++v) {
    const ViewSpec& V = G.view[v];
    const int spre_w = ceil_half(std::max(V.kw[0], V.kw[1]) - 1), spre_h = ceil_half(std::max(V.kh[0], V.kh[1]) - 1);
    int x0[3], y0[3], ox = 1 << 30, oy = 1 << 30;
    for (int k = 0; k < 3; ++k) {
      x0[k] = spre_w - V.kw[k] / 2;
      y0[k] = spre_h - V.kh[k] / 2;
      ox = std::min(ox, x0[k]);
      oy = std::min(oy, y0[k]);
    }
    int eh = 0, ew = 0;
    for (int k = 0; k < 3; ++k) {
      LmDet& D = K.det[3 * v + k];
      D.view = v;
      D.kind = k == 2 ? 1 : 0;
      D.list = k == 2 ? v : 2 * v + k;
      D.kh = V.kh[k];
      D.kw = V.kw[k];
      D.kwp = (D.kw + LM_JC - 1) / LM_JC * LM_JC;
      D.kw_ring = D.kw;
      D.w_off = w_off;
      w_off += D.kh * D.kwp;
      D.delta = G.delta[3 * v + k];
      D.oh = V.oh;
      D.ow = k == 2 ? std::min(tw, V.ow) : V.ow;
      D.in_y = y0[k] - oy;
      D.in_x = x0[k] - ox + G.xshift;
      D.m_y = spre_h - oy;
      D.m_x = spre_w - ox + G.xshift;
      D.tile_w = LM_TW;
      D.tile_h = 16;
      D.tiles_x = (D.ow + D.tile_w - 1) / D.tile_w;
      D.tiles_y = (D.oh + D.tile_h - 1) / D.tile_h;
      eh = std::max(eh, D.in_y + (G.tight ? D.oh : D.tiles_y * D.tile_h) + D.kh - 1);
      ew = std::max(ew, D.in_x + (D.tiles_x - 1) * D.tile_w + LM_TW + D.kwp - 1 + 4);
    }
    K.ext_h[v] = eh;
    K.ext_w[v] = (ew + 15) / 16 * 16;
  }
  int o = 0;
  for (int v = 0; v < 2; ++v) {
    K.fl_tx[v] = (G.view[v].ow + LM_FW - 1) / LM_FW;
    K.fl_ty[v] = (G.view[v].oh + LM_FH - 1) / LM_FH;
    K.fl_off[v] = o;
    o += (K.fl_tx[v] * K.fl_ty[v] + 3) / 4 * 4;
  }
  K.fl_slot = o;
  return w_off;
}

struct Region {
  const char* name;
  int64_t begin, used;  // byte offset; bytes the kernel touches there at most
};

// k_tile_bound_ref's LDS of view v.
void check_ref_lds(const LmConst& K, int v) {
  const int nbw = K.ext_w[v] / LM_TB_BLK;
  // k_tile_bound_ref: "uint8_t* bmin = bmax + eh * nbw" -- the view's block ranges come first
  int64_t end = 2 * (int64_t)K.ext_h[v] * nbw;
  bool any = false;
  for (int d : {3 * v + 2, 3 * v, 3 * v + 1}) {
    if (!K.tb_skip[d]) continue;
    any = true;
    const LmDet& D = K.det[d];
    const int ftx = D.kind != 0 ? K.tt_tx[v] : K.fl_tx[v];
    // k_tile_bound_ref: "rmax = tb_lds + K.tb_rng[d]; rmin = rmax + rows * ftx", rows * ftx entries each
    check(K.tb_rng[d] >= end, "ref: row ranges behind the block ranges and the detector before", K.tb_rng[d], end);
    end = K.tb_rng[d] + 2 * (int64_t)(D.oh + D.kh - 1) * ftx;
    // k_tile_bound_ref: "bmax[(D.in_y + r) * nbw + b]" for r < rows, b < lm_tb_blocks' end
    check(D.in_y >= 0 && D.in_y + D.oh + D.kh - 1 <= K.ext_h[v], "ref: window rows inside the ext crop");
    check(D.in_x >= 0 && D.in_x + D.ow + D.kw - 1 <= K.ext_w[v], "ref: window columns inside the ext crop");
  }
  check(any ? end <= K.tb_lds[v] : K.tb_lds[v] == 0, "ref: regions inside tb_lds", end, K.tb_lds[v]);
  check(K.tb_lds[v] <= kTbRefLds, "ref: tb_lds within 144 KB", K.tb_lds[v]);
}

// k_tile_bound's LDS and every band of view v.
void check_view(const LmConst& K, const LmTilePlan& plan, int v) {
  ++T.views;
  const int nbw = K.ext_w[v] / LM_TB_BLK;
  bool on[3], use[3], refine[3];
  int ftx[3], ty[3], sum_tx = 0, max_ty = 0;
  bool pairs = false;
  for (int k = 0; k < 3; ++k) {
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    // "on[k] = tail[k] ? tt_cnt != nullptr : pt_cnt != nullptr" (the host passes them by the effective switches)
    on[k] = D.kind != 0 ? plan.tailskip : plan.pointskip;
    use[k] = on[k] && K.tbw_use[d] != 0;  // "use[k] = on[k] && K.tbw_use[d] != 0"
    refine[k] = use[k] && K.tbr_on[d] != 0;
    pairs = pairs || refine[k];
    ftx[k] = D.kind != 0 ? K.tt_tx[v] : K.fl_tx[v];
    ty[k] = D.kind != 0 ? K.tt_ty[v] : K.fl_ty[v];
    if (on[k]) {
      sum_tx += ftx[k];
      max_ty = std::max(max_ty, ty[k]);
    }
    check(!K.tbw_use[d] || on[k], "a used detector is listed");
    check(!K.tbw_use[d] || K.tb_skip[d], "a used detector has a bound");
    // "if (use[k] && tid < 2 * K.det[3 * v + k].kh) pnv[k] = tbc[...]": one thread per P_i, N_i
    check(!use[k] || 2 * D.kh <= LM_TB_THREADS, "2 kh <= LM_TB_THREADS", D.kh);
    // "const int w = lm_div(e, rc)", "ty = lm_div(j, TBW_SEL(inv3))", "ty = lm_div(tile, K.tbw_inv[d])"
    check(K.tbw_inv[d] == lm_rcp(ftx[k]), "tbw_inv == lm_rcp(ftx)");
    bool div_ok = true;
    for (int j = 0; j < ftx[k] * ty[k]; ++j) div_ok = div_ok && lm_div(j, K.tbw_inv[d]) == j / ftx[k];
    check(div_ok, "lm_div(j, tbw_inv) == j / ftx over the grid");
  }
  const int br = K.tbw_br[v], nband = K.tbw_nband[v], rows = K.tbw_rows[v], blo = K.tbw_blo[v], nbk = K.tbw_nbk[v];
  const int nw = nbk / 2;
  // "(int)blockIdx.y < K.tbw_nband[0]" hands a band to every tile row of every listed grid
  check(br >= 1 && nband >= 1 && (int64_t)nband * br >= max_ty, "tbw_nband x tbw_br covers the tallest listed grid", nband * br, max_ty);
  // "const int nbk = K.tbw_nbk[v], nw = nbk / 2": a 32-bit word holds blocks 2 w and 2 w + 1 of k_ingest's ranges
  check(blo % 2 == 0 && nbk % 2 == 0, "tbw_blo and tbw_nbk even", blo, nbk);
  check(blo >= 0 && blo + nbk <= nbw, "the blocks lie inside the view's", blo + nbk, nbw);

  // ---- the regions, in order, with what the kernel touches of each at most
  std::vector<Region> R;
  R.push_back({"block ranges", 0, 2 * (int64_t)rows * nbk});  // "B[e] = w[u]" for e < nrow * nw
  check(K.tbw_v[v] % 4 == 0, "tbw_v at 4 bytes");              // "uint32_t* V = ...(tbw_lds + K.tbw_v[v])"
  // "V[e] = range_merge(...)" for e < (nrow - 3) * nw; refined: + a spare row and 16 bytes (checked per block below)
  R.push_back({"windows", K.tbw_v[v], 2 * (int64_t)std::max(0, rows - (LM_TB_H - 1)) * nbk + (pairs ? 2 * (int64_t)nbk + 16 : 0)});
  check(K.tbw_al[v] % 2 == 0, "tbw_al at 2 bytes");  // "uint16_t* AL = ...(tbw_lds + K.tbw_al[v])"
  // "AL[k * als + r]", als = tbw_rows, k < 3
  if (pairs) R.push_back({"last-block entries", K.tbw_al[v], 2 * 3 * (int64_t)rows});
  for (int k = 0; k < 3; ++k) {
    const int d = 3 * v + k;
    check(K.tbw_pn[d] % 8 == 0, "tbw_pn at 8 bytes");  // "reinterpret_cast<double*>(tbw_lds + K.tbw_pn[...])[tid]"
    if (use[k]) R.push_back({"P_i, N_i", K.tbw_pn[d], 16 * (int64_t)K.det[d].kh});
  }
  for (int k = 0; k < 3; ++k)  // "wmax = tbw_lds + K.tbw_win[d]; wmin = wmax + K.tbw_wsz[d]"
    if (use[k]) R.push_back({"window table", K.tbw_win[3 * v + k], 2 * (int64_t)K.tbw_wsz[3 * v + k]});
  for (int k = 0; k < 3; ++k) {
    check(K.tbw_ent[3 * v + k] % 4 == 0, "tbw_ent at 4 bytes");  // "reinterpret_cast<uint32_t*>(tbw_lds + K.tbw_ent[...])[pos]"
    if (on[k]) R.push_back({"entries", K.tbw_ent[3 * v + k], 4 * (int64_t)br * ftx[k]});
  }
  check(K.tbw_work[v] % 4 == 0, "tbw_work at 4 bytes");  // "uint32_t* work = ...(tbw_lds + K.tbw_work[v])"
  R.push_back({"work list", K.tbw_work[v], 4 * (int64_t)br * sum_tx});
  for (size_t i = 0; i < R.size(); ++i) {
    const int64_t next = i + 1 < R.size() ? R[i + 1].begin : K.tbw_lds[v];
    check(R[i].begin >= 0 && R[i].begin + R[i].used <= next, R[i].name, R[i].begin + R[i].used, next);
  }
  check(K.tbw_lds[v] <= kTbwLds, "tbw_lds within 64 KB", K.tbw_lds[v]);
  const int64_t v_end = K.tbw_al[v];  // where the windows, their spare row and 16 bytes end

  // ---- per detector: the blocks its window touches
  int first_blk = nbw;
  for (int k = 0; k < 3; ++k) {
    if (!use[k]) continue;
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    first_blk = std::min(first_blk, D.in_x / LM_TB_BLK);
    T.residues |= 1u << (D.in_x % LM_TB_BLK);
    T.rem[D.oh % LM_TB_H] += 1;
    const int lastw = D.ow - (ftx[k] - 1) * LM_TB_W;  // output columns of the last tile column
    if (lastw <= LM_TB_BLK) ++T.lastcol[1];
    else if (lastw <= 2 * LM_TB_BLK) ++T.lastcol[2];
    if (D.kh > LM_FH * br) ++T.tall;
    if (D.kh == 1) ++T.onerow;
    if (D.kw == 9) ++T.w9;
    if (D.kw == 70) ++T.w70;
    // "(the host accepts a bound only when the window lies inside the ext crop)": src rows y_lo .. of rng
    check(D.in_y >= 0 && D.in_y + D.oh + D.kh - 1 <= K.ext_h[v], "window rows inside the ext crop");
    for (int tx = 0; tx < ftx[k]; ++tx) {
      int c0, c1, b0, b1;
      lm_tb_span(tx, D.kw, D.ow, &c0, &c1);
      lm_tb_blocks(D.in_x, c0, c1, &b0, &b1);
      // "b0 = max(b0 - K.tbw_blo[v], 0); b1 = min(b1 - K.tbw_blo[v], nbk)": the clamps must not bite
      check(b0 >= blo && b1 <= blo + nbk && b0 < b1, "a tile column's blocks inside [tbw_blo, + tbw_nbk)", tx, b1);
    }
    // "bl = lm_tbr_block_end(...) - K.tbw_blo[v] - 1", "bendl = lm_tbr_block_end(...) - K.tbw_blo[v]", "bl0 = lm_tbr_block0(D.in_x, 0) - K.tbw_blo[v]"
    const int bendl = lm_tbr_block_end(D.in_x, D.ow, D.kw, nbw) - blo;
    check(bendl >= 1 && bendl <= nbk, "the window's last block inside the table", bendl, nbk);
    check(lm_tbr_block0(D.in_x, 0) - blo >= 0, "the window's first block inside the table");
  }

  if (first_blk < nbw && first_blk % 2 != 0) ++T.oddblk;

  // ---- every band, as the kernel's workgroup sees it
  // (a view lower than the tile rows a band would take: one band, of all its rows)
  if (sum_tx > 0 && nband == 1 && max_ty < std::max(1, LM_TBW_TILES / sum_tx)) ++T.low;
  for (int band = 0; band < nband; ++band) {
    ++T.bands;
    int t0[3], nt[3], ohb[3], nty[3];
    bool useb[3];
    int y_lo = K.ext_h[v], y_hi = 0;
    for (int k = 0; k < 3; ++k) {
      const LmDet& D = K.det[3 * v + k];
      ohb[k] = lm_tbw_band(D, ty[k], br, band, &t0[k], &nty[k]);
      nt[k] = on[k] ? nty[k] * ftx[k] : 0;
      useb[k] = use[k] && nt[k] > 0;  // "use[k] = use[k] && nt[k] > 0"
      if (useb[k]) {
        y_lo = std::min(y_lo, D.in_y + LM_FH * t0[k]);
        y_hi = std::max(y_hi, D.in_y + LM_FH * t0[k] + ohb[k] + D.kh - 1);
      }
    }
    y_hi = std::min(y_hi, K.ext_h[v]);
    // "const int nrow = max(0, min(y_hi - y_lo, K.tbw_rows[v]))": the clamp must not bite
    check(y_hi - y_lo <= rows, "the band's rows within tbw_rows", y_hi - y_lo, rows);
    const int nrow = std::max(0, std::min(y_hi - y_lo, rows));
    const int nvr = std::max(nrow - (LM_TB_H - 1), 0);
    // "work[pos] = ...": pos < nt[0] + nt[1] + nt[2]; "mark[t] = 0u" for t < nref <= the same
    check(4 * (int64_t)(nt[0] + nt[1] + nt[2]) <= K.tbw_lds[v] - K.tbw_work[v], "the band's tiles fit tbw_work");
    for (int k = 0; k < 3; ++k) {
      const int d = 3 * v + k;
      const LmDet& D = K.det[d];
      if (on[k]) {
        // "reinterpret_cast<uint32_t*>(tbw_lds + K.tbw_ent[3 * v + kk])[pos]": pos < nt[k]
        int64_t next = K.tbw_work[v];
        for (int kk = k + 1; kk < 3; ++kk)
          if (on[kk]) {
            next = K.tbw_ent[3 * v + kk];
            break;
          }
        check(K.tbw_ent[d] + 4 * (int64_t)nt[k] <= next, "the band's tiles fit tbw_ent", nt[k]);
      }
      if (!useb[k]) continue;
      const int wr = lm_tb_win_rows(ohb[k], D.kh);
      // "const int nent = min(lm_tb_win_rows(ohb[k], D.kh) * ftx[k], K.tbw_wsz[d])": the clamp must not bite
      check(K.tbw_wsz[d] >= wr * ftx[k], "tbw_wsz >= lm_tb_win_rows(ohb, kh) ftx", K.tbw_wsz[d], wr * ftx[k]);
      const int yb = D.in_y + LM_FH * t0[k] - y_lo;  // "const int yb = D.in_y + LM_FH * t0[k] - y_lo"
      check(yb >= 0, "the band's window row 0 among the loaded rows");
      for (int w = 0; w < wr; ++w) {
        int r0, nr;
        lm_tb_win_src(ohb[k], D.kh, w, &r0, &nr);
        // "const uint16_t* row = (nr == LM_TB_H ? V16 : B16) + (yb + r0) * nbk", nrr rows from there
        if (nr == LM_TB_H) check(yb + r0 < nvr, "a window-table row reads a four-row window that exists", yb + r0, nvr);
        else check(yb + r0 + nr <= nrow, "a window-table row reads block-range rows that exist", yb + r0 + nr, nrow);
      }
      // "lm_tb_tile_skip_win(wmax, wmax + wsz, fx, kh, lm_tb_win_row0(ohb, kh, ty), tx, ...)": rows row0 .. row0 + kh - 1
      for (int tyb = 0; tyb < nty[k]; ++tyb)
        check(lm_tb_win_row0(ohb[k], D.kh, tyb) + D.kh <= wr, "a tile's window-table rows exist", tyb);
      if (!refine[k]) continue;
      // 4b, per (tile, output block) of the band
      const int ng = K.tbr_ng[d], nc = lm_tbr_chunks(ng);
      check(ng == lm_tbr_groups(D.in_x, D.kw), "tbr_ng");
      const int bl0 = lm_tbr_block0(D.in_x, 0) - blo;
      const int nbx = (D.ow + LM_TB_BLK - 1) / LM_TB_BLK;
      for (int tyb = 0; tyb < nty[k]; ++tyb) {
        const int nr = std::min(LM_TB_H, ohb[k] - LM_TB_H * tyb);  // "const int nr = min(LM_TB_H, ohk - LM_TB_H * tyb)"
        const int row0 = yb + LM_TB_H * tyb;                         // "const int row0 = yb + LM_TB_H * tyb, ba0 = bl0 + xb"
        if (nr == LM_TB_H) {
          // level_v: "alone = AL + k * als + row0", one entry per weight row and one fetched ahead
          check(row0 + D.kh < rows, "the last-block entries reach a row past the last weight row", row0 + D.kh, rows);
          check(row0 + D.kh - 1 < nvr, "a term's four-row window exists", row0 + D.kh - 1, nvr);
          // "pw = V + row0 * nw + (ba0 >> 1)"; a chunk reads pw[0 .. 2]; "pw += lastc ? nw - 2 * (nc - 1) : 2" and the
          // fetch behind the last chunk of the last weight row: three words of row row0 + kh
          const int ba_max = bl0 + nbx - 1;
          const int64_t in_row = (int64_t)(row0 + D.kh - 1) * nw + (ba_max >> 1) + 2 * (nc - 1) + 2;
          const int64_t ahead = (int64_t)(row0 + D.kh) * nw + (ba_max >> 1) + 2;
          check(K.tbw_v[v] + 4 * (std::max(in_row, ahead) + 1) <= v_end, "the pair table's read-ahead inside the spare space",
                K.tbw_v[v] + 4 * (std::max(in_row, ahead) + 1), v_end);
        } else {
          // level_b: "row = B16 + (row0 + rs + i) * nbk", nn = nr rows from there, i < kh
          check(row0 + D.kh - 1 + nr <= nrow, "a short tile row's block-range rows exist", row0 + D.kh - 1 + nr, nrow);
        }
      }
    }
  }

  // ---- what the view kept, and the order of what it lost
  bool cand[3];
  for (int k = 0; k < 3; ++k)
    cand[k] = on[k] && K.tb_skip[3 * v + k] != 0 && 2 * K.det[3 * v + k].kh <= LM_TB_THREADS;
  for (int k = 0; k < 3; ++k) T.lost += cand[k] && !use[k] ? 1 : 0;
  // the snout loses its bound first, then the paw, the tail last
  check(!(cand[0] && cand[1] && use[1]) || use[0], "the paw keeps its bound while the snout does");
  check(!(cand[2] && (use[0] || use[1])) || use[2], "the tail keeps its bound while a point detector does");
  const LmTbwView W = lm_tbw_view(K, v, plan.tailskip, plan.pointskip);
  for (int k : {2, 0, 1}) {  // the last one dropped would not have fitted
    if (!cand[k] || use[k]) continue;
    bool again[3] = {use[0], use[1], use[2]};
    again[k] = true;
    check(lm_tbw_layout(K, W, again).lds > kTbwLds, "a detector loses its bound only when the band does not fit", k);
    break;
  }
  if (cand[0] && cand[1] && cand[2]) {
    if (use[0] && !use[1] && use[2]) ++T.keep101;
    if (!use[0] && !use[1] && use[2]) ++T.keep001;
  }
  bool one = false, any = false;
  for (int k = 0; k < 3; ++k) {
    any = any || refine[k];
    one = one || (refine[k] && lm_tbr_chunks(K.tbr_ng[3 * v + k]) == 1);
  }
  ++(one ? T.rowloop : any ? T.generic : T.unrefined);
}

void check_constants(const LmConst& K, const LmTilePlan& plan) {
  std::vector<std::pair<int64_t, int64_t>> iv;
  for (int d = 0; d < LM_NDET; ++d) {
    const LmDet& D = K.det[d];
    // "pnv[k] = tbc[K.tb_off[3 * v + k] + tid]" for tid < 2 kh; "C = tbc + K.tbr_off[d]", lm_tbr_const_size doubles
    iv.push_back({K.tb_off[d], K.tb_off[d] + 2 * (int64_t)D.kh});
    if (K.tbr_on[d]) iv.push_back({K.tbr_off[d], K.tbr_off[d] + (int64_t)lm_tbr_const_size(D.kh, K.tbr_ng[d])});
    check(K.tbr_off[d] % 8 == 0, "tbr_off a multiple of 8 doubles", K.tbr_off[d]);  // (a chunk is fetched as 64 aligned bytes)
  }
  std::sort(iv.begin(), iv.end());
  for (size_t i = 0; i < iv.size(); ++i) {
    check(iv[i].first >= 0 && iv[i].second <= (int64_t)plan.tbc.size(), "constants inside tbc", iv[i].second);
    check(i == 0 || iv[i].first >= iv[i - 1].second, "constants disjoint", iv[i].first);
  }
}

void check_switches(const LmConst& K, const LmTilePlan& plan, const Geom& G) {
  const LmTileSwitches& sw = G.sw;
  const bool list_ok = G.nslots <= 65535;  // (the grids themselves stay below 65,536 tiles here)
  check(plan.tailskip == (sw.tailskip && !sw.f16 && list_ok), "the effective tail skip");
  check(plan.pointskip == (sw.pointskip && !sw.f16 && sw.dark && list_ok), "the effective point skip");
  if (!plan.tailskip || !plan.pointskip || !sw.refine) ++T.off;
  bool one = false;
  for (int d = 0; d < LM_NDET; ++d) {
    const LmDet& D = K.det[d];
    const bool on = D.kind != 0 ? plan.tailskip : plan.pointskip;
    if (!on) check(!K.tb_skip[d] && !K.tbw_use[d] && !K.tbr_on[d], "a skip that is off leaves no bound", d);
    if (!sw.refine) check(!K.tbr_on[d], "no refinement with the refinement off", d);
    check(!K.tbr_on[d] || K.tb_skip[d], "a refined detector has a bound", d);
    if (!(D.delta < 0.f)) {
      ++T.nobound;
      check(!K.tb_skip[d] && !K.tbw_use[d] && !K.tbr_on[d], "delta >= 0: no bound", d);
    }
    one = one || (K.tbw_use[d] && K.tbr_on[d] && lm_tbr_chunks(K.tbr_ng[d]) == 1);
  }
  check(plan.row_loop == (LM_TBW_ROW_LOOP && one), "the row-loop flag");
  check(plan.tb_lds == (size_t)std::max(K.tb_lds[0], K.tb_lds[1]), "tb_lds: the larger view's");
  check(plan.tbw_lds == (size_t)std::max(K.tbw_lds[0], K.tbw_lds[1]), "tbw_lds: the larger view's");
}

void run(const Geom& G) {
  ++T.geoms;
  LmConst K;
  const int w_off = fill_inputs(K, G);
  // small seeded weights
  std::vector<float> wts((size_t)w_off, 0.f);
  uint64_t s = 20240917u + (uint64_t)T.geoms;
  for (int d = 0; d < LM_NDET; ++d) {
    const LmDet& D = K.det[d];
    for (int i = 0; i < D.kh; ++i)
      for (int j = 0; j < D.kw; ++j) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        wts[(size_t)D.w_off + i * D.kwp + j] = (float)((int)((s >> 33) % 2001u) - 1000) / (1000.0f * (float)(D.kh * D.kw));
      }
  }
  const LmTilePlan plan = lm_tile_plan(K, G.nslots, wts.data(), G.sw);
  g_where = G.name;
  check_switches(K, plan, G);
  check_constants(K, plan);
  for (int v = 0; v < 2; ++v) {
    g_where = std::string(G.name) + (v ? " side" : " bottom");
    check_ref_lds(K, v);
    check_view(K, plan, v);
  }
}

Geom scaled(const char* name, int s) {  // synthetic.py's detectors and default boxes at scale s
  Geom G;
  G.name = name;
  G.view[0] = {140 * s, 400 * s, {24 * s, 30 * s, 16 * s}, {24 * s, 30 * s, 26 * s}};
  G.view[1] = {90 * s, 400 * s, {22 * s, 26 * s, 16 * s}, {22 * s, 26 * s, 26 * s}};
  return G;
}

}  // namespace

int main() {
  std::vector<Geom> all;
  all.push_back(scaled("C3", 1));
  all.push_back(scaled("C5", 2));  // two chunks of group constants per weight row: the generic loop
  {  // the switches, on C3
    const LmTileSwitches sws[] = {{false, true, true, false, true}, {true, false, true, false, true}, {true, true, false, false, true},
                                  {true, true, true, true, true},  {true, true, true, false, false}, {false, false, true, false, true}};
    for (const LmTileSwitches& sw : sws) {
      Geom G = scaled("C3 switches", 1);
      G.sw = sw;
      all.push_back(G);
    }
    Geom G = scaled("C3 65,536 slots", 1);
    G.nslots = 65536;
    all.push_back(G);
    G = scaled("C3 delta >= 0", 1);
    G.delta[DET_SNOUT_B] = 0.f;
    G.delta[DET_TAIL_S] = 2.f;
    all.push_back(G);
  }
  // boxes lower than one band of tile rows; last tile rows of 1, 2, 3 output rows; tight ext crops
  for (int oh : {1, 2, 3, 5, 6, 7, 9, 18, 27})
    for (int tight = 0; tight < 2; ++tight) {
      Geom G = scaled("low box", 1);
      G.view[0].oh = oh;
      G.view[1].oh = oh + 40;
      G.tight = tight != 0;
      all.push_back(G);
    }
  // a detector taller than a band; a one-row detector; widths 9 and 70; every in_x mod 8; last tile columns of one
  // and two blocks (ow mod 40 in 1 .. 16); a first block that is odd (xshift 8 .. 15)
  for (int xs = 0; xs < 2 * LM_TB_BLK; ++xs)
    for (int ow : {41, 48, 49, 56, 200, 401, 409}) {
      Geom G = scaled("odd sizes", 1);
      G.xshift = xs;
      G.view[0] = {23 + xs, ow, {1, 70, 9}, {9, 70, 70}};
      G.view[1] = {37, ow + 3, {120, 3, 1}, {11, 9, 33}};
      G.tight = (xs & 1) != 0;
      if (xs == 7) G.view[1].kh[0] = 130;  // more weight rows than LM_TB_THREADS / 2: no bound in k_tile_bound
      all.push_back(G);
    }
  // wide boxes up to LM_INGEST_MAXTX tile columns: detectors lose their bound to the 64 KB
  for (int ow : {3000, 4000, 4400, LM_INGEST_MAXTX * LM_FW - 7, LM_INGEST_MAXTX * LM_FW}) {
    Geom G = scaled("wide box", 1);
    G.view[0].ow = G.view[1].ow = ow;
    all.push_back(G);
    G.view[0].oh = 1;
    G.view[1].kh[1] = 60;
    all.push_back(G);
  }
  for (const Geom& G : all) run(G);
  int nres = 0;
  for (int r = 0; r < LM_TB_BLK; ++r) nres += (T.residues >> r) & 1u;
  std::printf(
      "%ld geometries, %ld views, %ld bands, %ld lost, %ld rowloop, %ld generic, %ld unrefined, %d residues, rem %ld %ld %ld, "
      "lastcol %ld %ld, tall %ld, onerow %ld, low %ld, w9 %ld w70 %ld, oddblk %ld, keep101 %ld keep001 %ld, off %ld, nobound %ld, %ld checks, "
      "%ld failures\n",
      T.geoms, T.views, T.bands, T.lost, T.rowloop, T.generic, T.unrefined, nres, T.rem[1], T.rem[2], T.rem[3], T.lastcol[1],
      T.lastcol[2], T.tall, T.onerow, T.low, T.w9, T.w70, T.oddblk, T.keep101, T.keep001, T.off, T.nobound, T.checks, T.fails);
  return T.fails == 0 ? 0 : 1;
}
