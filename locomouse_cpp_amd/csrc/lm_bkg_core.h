// lm_bkg_core.h — the background estimate's arithmetic (include/locomouse_bkg.h),
// compiled for host and device: the rank of a permille, one sample's (or one
// run of equal samples') update of a pixel's 256-bin histogram, and the
// selection of the value at a rank from it.  Integers only.
//
// A pixel's histogram is 256 counters of lmb_count (16 bits), bin v counting
// the samples of value v; the pixels' histograms follow one another
// (hist[pixel][256]).  No counter passes LMB_MAX_SAMPLES because the caller
// refuses the push that would take the sample count past it.
#ifndef LM_BKG_CORE_H
#define LM_BKG_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LMB_HD __host__ __device__ inline
#else
#define LMB_HD inline
#endif

typedef uint16_t lmb_count;
#define LMB_BINS 256
#define LMB_MAX_SAMPLES 65535  // the largest lmb_count (LM_BKG_MAX_SAMPLES)

// Zero-based index, in a pixel's K >= 1 samples sorted ascending, of the value
// `permille` (0..1000) selects: 500 is the lower median.
LMB_HD uint32_t lmb_rank(int32_t permille, int64_t K) { return (uint32_t)(((int64_t)permille * (K - 1)) / 1000); }

// A run of equal samples of one pixel, kept in registers until the value
// changes (a background pixel mostly repeats itself), then added in one update.
struct LmbRun {
  uint32_t value, length;  // length 0: no run yet
};

LMB_HD void lmb_flush(lmb_count* h, LmbRun& r) {
  if (r.length) h[r.value] = (lmb_count)(h[r.value] + r.length);
  r.length = 0;
}

LMB_HD void lmb_push(lmb_count* h, LmbRun& r, uint32_t v) {
  if (r.length && r.value == v) {
    ++r.length;
    return;
  }
  lmb_flush(h, r);
  r.value = v;
  r.length = 1;
}

// The value at zero-based index `rank` of the sorted samples h counts: the
// first bin at which the running sum passes rank.  rank is below the number of
// samples; were it not, the last bin is the answer (no index leaves h).
LMB_HD uint8_t lmb_select(const lmb_count* h, uint32_t rank) {
  uint32_t sum = 0;
  for (int v = 0; v < LMB_BINS - 1; ++v) {
    sum += h[v];
    if (sum > rank) return (uint8_t)v;
  }
  return (uint8_t)(LMB_BINS - 1);
}

// ---- the host statement (CPU tests; the library's kernels do the same per pixel)

// Adds n frames (frame i at frames + i * pitch, npix u8) to hist[npix][256].
inline void lmb_host_accumulate(lmb_count* hist, const uint8_t* frames, int64_t pitch, int32_t n, size_t npix) {
  for (size_t p = 0; p < npix; ++p) {
    lmb_count* h = hist + p * LMB_BINS;
    LmbRun r{0, 0};
    for (int32_t i = 0; i < n; ++i) lmb_push(h, r, frames[(int64_t)i * pitch + (int64_t)p]);
    lmb_flush(h, r);
  }
}

inline void lmb_host_select(const lmb_count* hist, size_t npix, int32_t permille, int64_t samples, uint8_t* out) {
  const uint32_t rank = lmb_rank(permille, samples);
  for (size_t p = 0; p < npix; ++p) out[p] = lmb_select(hist + p * LMB_BINS, rank);
}

#endif  // LM_BKG_CORE_H
