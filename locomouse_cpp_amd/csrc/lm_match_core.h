/*
 * lm_match_core.h — histogram matching of the bottom crop to a reference
 * image's cumulative histogram, as use_reference_image_brightness intends it
 * (cropBoundingBox, LocoMouse_class.cpp:1437-1443; histogramMatching,
 * :3313-3387; computeNormalizedCDF, :3389-3414).  One definition for the host
 * (lm_match_cdf, tests/cpp/match_check.cpp) and the device (k_match runs the
 * two serial parts on one lane per slot); build with -ffp-contract=off.
 *
 *   histogram  h[256]: exact 32-bit counts of the n = rows cols pixels
 *   CDF        p[i] = (float)h[i] * (float)(1.0 / (double)n)   (hist / (cols * rows) as convertTo evaluates it),
 *              c[0] = p[0], c[i] = c[i - 1] + p[i] in float, in index order
 *   table      the two loops of :3351-3380, literally (lm_match_table)
 */
#ifndef LM_MATCH_CORE_H
#define LM_MATCH_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LM_MATCH_HD __host__ __device__ inline
#else
#define LM_MATCH_HD inline
#endif

// (float)(1.0 / (double)n): the factor of hist / (cols * rows)
LM_MATCH_HD float lm_match_scale(int64_t n) { return (float)(1.0 / (double)n); }

// c[256] from h[256] (h and c may live in any address space the caller's
// pointers reach; c is written in index order and c[i - 1] read back)
template <class H, class CP>
LM_MATCH_HD void lm_match_cdf_of(const H* h, float scale, CP* c) {
  float acc = (float)h[0] * scale;
  c[0] = acc;
  for (int i = 1; i < 256; ++i) {
    const float p = (float)h[i] * scale;
    acc = acc + p;
    c[i] = acc;
  }
}

// T[256] from the image's CDF c and the reference's ref.  Returns the number
// of entries the second loop (no ref[j] >= c[i] from cur on) decided.
template <class CP, class RP, class TP>
LM_MATCH_HD int lm_match_table(const CP* c, const RP* ref, TP* T) {
  int cur = 0, fallback = 0;
  for (int i = 0; i < 256; ++i) {
    const float ci = c[i];
    bool assigned = false;
    for (int j = cur; j < 256; ++j)
      if (ref[j] >= ci) {
        T[i] = (uint8_t)j;
        cur = j;
        assigned = true;
        break;
      }
    if (!assigned) {
      float min_diff = 1.0f;
      for (int j = cur; j < 256; ++j) {
        const float d = ci - ref[j];
        if (d < min_diff) {
          min_diff = d;
          cur = j;
        }
      }
      T[i] = (uint8_t)cur;
      ++fallback;
    }
  }
  return fallback;
}

// h[256] of a rows x cols image with row pitch `pitch` bytes (host)
inline void lm_match_hist(const uint8_t* image, int32_t rows, int32_t cols, int64_t pitch, uint32_t* h) {
  for (int i = 0; i < 256; ++i) h[i] = 0u;
  for (int32_t r = 0; r < rows; ++r) {
    const uint8_t* p = image + (int64_t)r * pitch;
    for (int32_t c = 0; c < cols; ++c) ++h[p[c]];
  }
}

// a reference CDF lm_ctx_create_matched takes: 256 finite, non-negative,
// non-decreasing floats; null, or what is wrong with it
inline const char* lm_match_cdf_bad(const float* cdf) {
  for (int i = 0; i < 256; ++i) {
    const float v = cdf[i];
    if (!(v == v) || v - v != 0.0f) return "reference_cdf: every entry must be finite.";
    if (v < 0.0f) return "reference_cdf: every entry must be non-negative.";
    if (i > 0 && v < cdf[i - 1]) return "reference_cdf: the entries must be non-decreasing.";
  }
  return nullptr;
}

#endif  // LM_MATCH_CORE_H
