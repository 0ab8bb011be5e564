/*
 * lm_corr_narrow.h — the narrow class of ring work items (plain C++ and HIP:
 * k_tile_bound, lm_corr.hip's narrow kernels and
 * tests/cpp/narrow_class_check.cpp share it; no HIP call, no environment).
 *
 * k_tile_bound's refinement proves a kept LM_FW x LM_FH tile per 8-column
 * output block (lm_tail_bound.h: lm_tbr_block_skip); the tile stays listed as
 * soon as one block is unproven.  Its block mask (bit b: block b unproven)
 * says which columns the correlation has to compute.  A tile whose unproven
 * blocks span at most LM_NW_SPAN blocks is *narrow*: it runs as a work item of
 * LM_NW_FW x LM_FH outputs (4 lanes of 5 columns x 4 rows, 16 items per wave)
 * at half the cost of the whole tile.  Every other listed tile is *wide* and
 * runs as before.
 *
 * A narrow item's origin is tile_x + min(8 first, LM_FW - LM_NW_FW): inside
 * its tile, a multiple of 4.  It owns the columns of its span only, clipped
 * to the detector's ow; the kernels drop every output outside them.
 */
#ifndef LM_CORR_NARROW_H
#define LM_CORR_NARROW_H

#include <stdint.h>

#include "lm_device.h"

#define LM_NW_FW 20                     // output columns of a narrow item
#define LM_NW_NQ (64 / (LM_NW_FW / 5))  // narrow items per wave
#define LM_NW_BLK 8                     // columns of an output block (LM_TB_BLK)
#define LM_NW_NBX (LM_FW / LM_NW_BLK)   // blocks per tile (LM_TB_NBX)
#define LM_NW_SPAN 2                    // widest span of a narrow tile, in blocks
#define LM_NW_UNTRIED 0x20u             // mask bit: the refinement did not try the tile per 4-row block
static_assert(LM_NW_SPAN * LM_NW_BLK <= LM_NW_FW && LM_NW_FW % 5 == 0 && (LM_FW - LM_NW_FW) % 4 == 0, "narrow item geometry");

#define LM_NW_FN LM_HD inline __attribute__((always_inline))

struct LmNwClass {
  int narrow;  // 1: a narrow item; 0: wide
  int first;   // first unproven block (narrow)
  int count;   // blocks of the span, first to last unproven (narrow)
};

// mask: bit b set = block b of the tile is unproven (bits 0 .. LM_NW_NBX - 1),
// LM_NW_UNTRIED: the tile was not refined per 4-row block (a detector without
// the refinement, a short last tile row).  A mask without a block bit belongs
// to no listed tile; it classifies as wide.
LM_NW_FN LmNwClass lm_nw_classify(uint32_t mask) {
  LmNwClass c{0, 0, 0};
  const uint32_t m = mask & ((1u << LM_NW_NBX) - 1u);
  if ((mask & LM_NW_UNTRIED) != 0u || m == 0u) return c;
  int first = 0, last = LM_NW_NBX - 1;
  while (!(m >> first & 1u)) ++first;
  while (!(m >> last & 1u)) --last;
  if (last - first + 1 > LM_NW_SPAN) return c;
  c.narrow = 1;
  c.first = first;
  c.count = last - first + 1;
  return c;
}

// The mask of a tile of nblocks blocks (a last tile column has fewer than
// LM_NW_NBX) from a predicate of its blocks -- unproven(b): block b is not
// proven (on the host: !lm_tbr_block_skip of the tile's rows); tried: the
// refinement takes the tile's rows as one 4-row block.  What k_tile_bound's
// step 4b leaves in an entry's mark word.
template <class F>
LM_NW_FN uint32_t lm_nw_mask_of(int nblocks, bool tried, F unproven) {
  uint32_t m = 0u;
  for (int b = 0; b < nblocks && b < LM_NW_NBX; ++b)
    if (unproven(b)) m |= (1u << b) | (tried ? 0u : LM_NW_UNTRIED);
  return m;
}

// The item's origin, in columns past its tile's.
LM_NW_FN int lm_nw_origin(int first) {
  const int o = LM_NW_BLK * first;
  return o < LM_FW - LM_NW_FW ? o : LM_FW - LM_NW_FW;
}

// The columns the item owns, [*x0, *x1) of the detector's outputs (tile_x: its tile's first column).
LM_NW_FN void lm_nw_owned(int tile_x, int first, int count, int ow, int* x0, int* x1) {
  *x0 = tile_x + LM_NW_BLK * first;
  const int e = tile_x + LM_NW_BLK * (first + count);
  *x1 = e < ow ? e : ow;
}

// A narrow list entry: the tile's entry of the existing lists (slot << 16 |
// tile) in the low word, first | count << 4 in the high one.
LM_NW_FN uint64_t lm_nw_entry(uint32_t tile_entry, int first, int count) {
  return (uint64_t)tile_entry | (uint64_t)(uint32_t)(first | count << 4) << 32;
}
LM_NW_FN uint32_t lm_nw_entry_tile(uint64_t e) { return (uint32_t)e; }
LM_NW_FN int lm_nw_entry_first(uint64_t e) { return (int)(e >> 32) & 15; }
LM_NW_FN int lm_nw_entry_count(uint64_t e) { return (int)(e >> 36) & 15; }

// ---- the new lists' counters, one buffer of LM_NW_CNT_WORDS words per lane:
// the wide lists' in the existing lists' layout (the ring kernels read them in
// place of those: per point list id, then per tail detector), then the narrow
// lists' per detector id
#define LM_NW_CNT_PTW 0
#define LM_NW_CNT_TTW (LM_NLIST * LM_TL_NC)
#define LM_NW_CNT_N ((LM_NLIST + 2) * LM_TL_NC)
#define LM_NW_CNT_WORDS ((LM_NLIST + 2 + LM_NDET) * LM_TL_NC)

// What k_tile_bound writes with the narrow class on (all null: off).  The wide
// lists have the existing lists' layout (ptw_list: list id l at l * tl_stride,
// ttw_list: tail detector t at t * tt_stride); n_list holds the narrow entries
// in the same places, the tail detectors' after the point lists'
// (LM_NLIST * tl_stride + t * tt_stride).
struct LmNarrowOut {
  int32_t* cnt;  // LM_NW_CNT_WORDS counters, zeroed by k_prep
  uint32_t* ptw_list;
  uint32_t* ttw_list;
  unsigned long long* n_list;
};

// ---- the narrow launches' wave directory: a narrow class has
// ceil(cnt / LM_NW_NQ) waves per segment, packed densely like the wide ones
// (lm_corr_dir.h); the record of a narrow launch group has that header's
// layout and is searched the same way
struct LmCorrDirRecN {
  int32_t end[LM_NDET];  // narrow waves of the group's detectors 0 .. k, cumulative
  int32_t total;
  int32_t pad;
};
static_assert(sizeof(LmCorrDirRecN) == 32, "one 32-byte scalar load");

LM_NW_FN int lm_nw_seg_waves(int cnt) { return (cnt + LM_NW_NQ - 1) / LM_NW_NQ; }
LM_NW_FN int lm_nw_listed_waves(const int32_t* cnt) {
  int w = 0;
  for (int c = 0; c < LM_TL_NC; ++c) w += lm_nw_seg_waves(cnt[c]);
  return w;
}
LM_NW_FN LmCorrDirRecN lm_nw_record(const int32_t* waves, int n) {
  LmCorrDirRecN r;
  int e = 0;
  for (int k = 0; k < LM_NDET; ++k) {
    if (k < n) e += waves[k];
    r.end[k] = e;
  }
  r.total = e;
  r.pad = 0;
  return r;
}
// Wave g of a narrow group of n detectors -> its detector's place and the wave's number in it; false: past the last.
LM_NW_FN bool lm_nw_lookup(const LmCorrDirRecN& r, int n, int g, int* k, int* local) {
  if (g >= r.total) return false;
  int kk = 0, base = 0;
  for (int j = 0; j < LM_NDET - 1; ++j)
    if (j + 1 < n && g >= r.end[j]) {
      kk = j + 1;
      base = r.end[j];
    }
  *k = kk;
  *local = g - base;
  return true;
}
// Wave `local` of a detector with segment counters cnt -> its segment *c, its place *w there and its items *nv.
LM_NW_FN bool lm_nw_segment(const int32_t* cnt, int local, int* c, int* w, int* nv) {
  int base = 0;
  for (int s = 0; s < LM_TL_NC; ++s) {
    const int wv = lm_nw_seg_waves(cnt[s]);
    if (local < base + wv) {
      *c = s;
      *w = local - base;
      const int left = cnt[s] - LM_NW_NQ * *w;
      *nv = left < LM_NW_NQ ? left : LM_NW_NQ;
      return true;
    }
    base += wv;
  }
  return false;
}
// Waves a narrow launch of a group is given (its grid): a segment of k slots
// lists at most 8 nt k items (the places of its nt 80 x 16 tiles), so at most
// ceil(nt k / 2) waves; the 64 segments' slots add up to the batch's.
LM_NW_FN int lm_nw_grid_waves(int tiles, int nslots, int ndet) { return (tiles * nslots + 1) / 2 + LM_TL_NC * ndet; }

#endif  // LM_CORR_NARROW_H
