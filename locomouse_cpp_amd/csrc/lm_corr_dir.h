/*
 * lm_corr_dir.h — the wave directory of a ring correlation launch (plain C++
 * and HIP: lm_corr.hip's corr_locate_rw and k_corr_dir and
 * tests/cpp/corr_dir_check.cpp share it; no HIP call, no environment).
 *
 * A ring launch (k_corr_rw, k_corr_rw_all) flattens the batch's work
 * detector-major: the waves of the group's first detector, then the next
 * one's.  A listed detector (its tiles come from 64 list segments) has
 * ceil(cnt / LM_RW_NQ) waves per segment, packed densely; an unlisted one has
 * one wave per 80 x 16 tile and slot.  The directory record of a group holds
 * the cumulative wave counts in the group's detector order, so wave g finds
 * its detector, or that it has none, from the record alone.
 */
#ifndef LM_CORR_DIR_H
#define LM_CORR_DIR_H

#include <stdint.h>

#include "lm_device.h"

// (always inlined: a call from a ring kernel would cost it its registers)
#define LM_CD_FN LM_HD inline __attribute__((always_inline))

// One launch group's record, 32 bytes (a wave reads it with one scalar load).
struct LmCorrDirRec {
  int32_t end[LM_NDET];  // waves of the group's detectors 0 .. k, cumulative (k >= n: the total)
  int32_t total;         // waves of the group
  int32_t pad;
};
static_assert(sizeof(LmCorrDirRec) == 32, "one 32-byte scalar load");

// Waves of one list segment of cnt tiles.
LM_CD_FN int lm_cd_seg_waves(int cnt) { return (cnt + LM_RW_NQ - 1) / LM_RW_NQ; }

// Waves of a listed detector: its LM_TL_NC segment counters.
LM_CD_FN int lm_cd_listed_waves(const int32_t* cnt) {
  int w = 0;
  for (int c = 0; c < LM_TL_NC; ++c) w += lm_cd_seg_waves(cnt[c]);
  return w;
}

// Waves of an unlisted detector of nt 80 x 16 tiles per slot.
LM_CD_FN int lm_cd_unlisted_waves(int nt, int nslots) { return nt * nslots; }

// The record from the waves of a group's n detectors.
LM_CD_FN LmCorrDirRec lm_cd_record(const int32_t* waves, int n) {
  LmCorrDirRec r;
  int e = 0;
  for (int k = 0; k < LM_NDET; ++k) {
    if (k < n) e += waves[k];
    r.end[k] = e;
  }
  r.total = e;
  r.pad = 0;
  return r;
}

// Wave g of a group of n detectors -> its detector's place k in the group and
// the wave's number within that detector; false: past the last wave.
LM_CD_FN bool lm_cd_lookup(const LmCorrDirRec& r, int n, int g, int* k, int* local) {
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

#endif  // LM_CORR_DIR_H
