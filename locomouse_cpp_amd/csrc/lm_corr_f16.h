// lm_corr_f16.h — the plan of k_corr_f16 (lm_corr.hip; the non-parity
// LM_CORR_F16 mode): the workgroup tile, the chunk count of a detector width,
// the f16 window's size in LDS and the host's layout of the B fragments.
// Shared by the kernel, the runtime (lm_runtime.hip: validate, the plans,
// f16_fragments) and a plain C++ compiler (tests/cpp/f16_plan_check.cpp).
#ifndef LM_CORR_F16_H
#define LM_CORR_F16_H

#include <stddef.h>
#include <stdint.h>

#include "lm_device.h"

// k_corr_f16 (non-parity LM_CORR_F16 mode): 2 x 2 waves per workgroup, each
// with two 32 x 32 accumulator tiles side by side -> a 128 x 64 output tile
// (round 4: 5 waves of 32 columns, -4 % k_corr at C5 but fewer frames/s;
// four 32-row tiles per wave, 130k vs 150k C5 frames/s at two waves per SIMD)
#define LM_F16_WAVES 4
#define LM_F16_TW 128
#define LM_F16_TH 64
#define LM_F16_THREADS (64 * LM_F16_WAVES)
#define LM_F16_MAX_NCH 10

LM_HD constexpr int f16_nch(int kw) { return (kw + 31 + 15) / 16; }
LM_HD constexpr int f16_cols(int nch) { return LM_F16_TW - 32 + 16 * nch; }
LM_HD constexpr int f16_stride(int cols) { return (cols + 7) / 16 * 16 + 8; }
LM_HD constexpr size_t f16_lds_bytes(int nch, int kh) {
  // the f16 window (the B fragments come from global memory)
  (void)nch;
  return (size_t)(LM_F16_TH + kh - 1) * f16_stride(f16_cols(nch)) * 2;
}
// Host: the B fragment of (row i, chunk c) for lane l, element j (0 off the band).
static inline float f16_bfrag_weight(const double* w, int kw, int i, int c, int l, int j) {
  const int r = l & 31, h = l >> 5, jj = 16 * c + 8 * h + j - r;
  return (jj >= 0 && jj < kw) ? (float)w[(size_t)i * kw + jj] : 0.0f;
}

#endif  // LM_CORR_F16_H
