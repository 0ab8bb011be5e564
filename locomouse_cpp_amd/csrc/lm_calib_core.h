// lm_calib_core.h — the calibration estimate (include/locomouse_calib.h) in
// plain C++: the per-view record's pieces that the kernel (lm_calib.hip) runs
// per pixel, the whole record on the host (lmc_host_record, what the tests
// compare the kernel with), and the fp64 fit and map, which run on the host
// only.  No HIP calls.  Every floating-point expression below is one rounded
// operation per operator, in the order written (the library and the host code
// are built with -ffp-contract=off), so a restatement in Python floats gives
// the same bits.
#ifndef LM_CALIB_CORE_H
#define LM_CALIB_CORE_H

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "locomouse_calib.h"

#if defined(__HIPCC__)
#define LMC_HD __host__ __device__ inline
#else
#define LMC_HD inline
#endif

// d = max(0, frame - background)
LMC_HD int lmc_diff(uint32_t f, uint32_t b) { return f > b ? (int)(f - b) : 0; }

// The key whose maximum over a view is its peak at the first position in
// row-major order: d above, the complement of the frame index (< 2^31) below.
LMC_HD uint64_t lmc_key(uint32_t d, uint32_t index) { return ((uint64_t)d << 32) | (uint64_t)(0xFFFFFFFFu - index); }
LMC_HD uint32_t lmc_key_peak(uint64_t key) { return (uint32_t)(key >> 32); }
LMC_HD uint32_t lmc_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// Rows [r0, r1) of view 0 (side) or 1 (bottom).
LMC_HD void lmc_view_rows(int view, int rows, int split_row, int* r0, int* r1) {
  *r0 = view ? split_row : 0;
  *r1 = view ? rows : split_row;
}

struct LmcWindow {
  int r0, r1, c0, c1;  // rows [r0, r1], columns [c0, c1], inside the view
  int clipped;
};

// The window of radius R about (px, py), intersected with the view's rows
// [vr0, vr1) and the frame's columns.
LMC_HD LmcWindow lmc_window(int px, int py, int R, int vr0, int vr1, int cols) {
  LmcWindow w;
  w.r0 = py - R < vr0 ? vr0 : py - R;
  w.r1 = py + R > vr1 - 1 ? vr1 - 1 : py + R;
  w.c0 = px - R < 0 ? 0 : px - R;
  w.c1 = px + R > cols - 1 ? cols - 1 : px + R;
  w.clipped = (py - R < vr0 || py + R > vr1 - 1 || px - R < 0 || px + R > cols - 1) ? 1 : 0;
  return w;
}

inline const char* lmc_check_opts(const lm_calib_opts& o) {
  if (o.threshold < 0 || o.threshold > 255) return "threshold must be in 0..255";
  if (o.radius < 0 || o.radius > LM_CALIB_MAX_RADIUS) return "radius must be in 0..LM_CALIB_MAX_RADIUS";
  if (o.min_peak < 0 || o.min_peak > 255) return "min_peak must be in 0..255";
  if (o.min_area < 1) return "min_area must be at least 1";
  if (o.max_stray < 0) return "max_stray must not be negative";
  return nullptr;
}

inline const char* lmc_check_shape(int64_t rows, int64_t cols, int64_t split_row) {
  if (rows <= 0 || cols <= 0 || rows > 65535 || cols > 65535) return "rows and cols must be in 1..65535";
  if (rows * cols >= (int64_t)1 << 31) return "rows * cols must be below 2^31";
  if (split_row < 1 || split_row >= rows) return "split_row must be in 1..rows-1";
  return nullptr;
}

// One view's record of one frame, on the host, as the kernel computes it.
inline void lmc_host_record(const uint8_t* frame, const uint8_t* bkg, int rows, int cols, int split_row, int view,
                            const lm_calib_opts& o, lm_calib_record* rec) {
  int vr0, vr1;
  lmc_view_rows(view, rows, split_row, &vr0, &vr1);
  uint64_t key = 0;
  int n_above = 0;
  for (uint32_t i = (uint32_t)vr0 * (uint32_t)cols; i < (uint32_t)vr1 * (uint32_t)cols; ++i) {
    const int d = lmc_diff(frame[i], bkg[i]);
    const uint64_t k = lmc_key((uint32_t)d, i);
    if (k > key) key = k;
    n_above += d > o.threshold;
  }
  const uint32_t idx = lmc_key_index(key);
  rec->peak = (int32_t)lmc_key_peak(key);
  rec->px = (int32_t)(idx % (uint32_t)cols);
  rec->py = (int32_t)(idx / (uint32_t)cols);
  rec->n_above = n_above;
  const LmcWindow w = lmc_window(rec->px, rec->py, o.radius, vr0, vr1, cols);
  rec->clipped = w.clipped;
  rec->n_in = 0;
  rec->S = rec->Sx = rec->Sy = 0;
  for (int r = w.r0; r <= w.r1; ++r)
    for (int c = w.c0; c <= w.c1; ++c) {
      const size_t i = (size_t)r * cols + c;
      const int d = lmc_diff(frame[i], bkg[i]);
      if (d > o.threshold) {
        rec->n_in += 1;
        rec->S += d;
        rec->Sx += (int64_t)d * c;
        rec->Sy += (int64_t)d * r;
      }
    }
}

// ---- the fit (host only)

LMC_HD bool lmc_view_ok(const lm_calib_record& r, const lm_calib_opts& o) {
  return r.peak >= o.min_peak && r.n_in >= o.min_area && r.n_above - r.n_in <= o.max_stray && r.clipped == 0;
}

struct LmcSample {
  int32_t frame;
  double xb, xs;
};

// The samples of records[n_frames][2] (side, bottom), in frame order.
inline void lmc_samples(const lm_calib_record* rec, int n_frames, const lm_calib_opts& o, std::vector<LmcSample>& out) {
  out.clear();
  for (int f = 0; f < n_frames; ++f) {
    const lm_calib_record &s = rec[2 * f], &b = rec[2 * f + 1];
    if (!lmc_view_ok(s, o) || !lmc_view_ok(b, o) || s.S <= 0 || b.S <= 0) continue;
    out.push_back(LmcSample{f, (double)b.Sx / (double)b.S, (double)s.Sx / (double)s.S});
  }
}

inline double lmc_t(double x, int cols) {
  const double half = (double)cols / 2.0;
  return (x - half) / half;
}

// p(t) and dp/dt by Horner's rule.
inline double lmc_poly(const double* coef, int degree, double t) {
  double p = coef[degree];
  for (int k = degree - 1; k >= 0; --k) p = p * t + coef[k];
  return p;
}
inline double lmc_poly_dt(const double* coef, int degree, double t) {
  double d = (double)degree * coef[degree];
  for (int k = degree - 1; k >= 1; --k) d = d * t + (double)k * coef[k];
  return d;
}

// Least squares of xs on the powers of t over the samples flagged in `use`,
// in order: normal equations, Cholesky without pivoting.  False when the
// matrix is not positive definite.
inline bool lmc_solve(const std::vector<LmcSample>& sm, const std::vector<char>& use, int cols, int degree, double* coef) {
  const int N = degree + 1;
  double M[2 * LM_CALIB_MAX_DEGREE + 1] = {0}, bv[LM_CALIB_MAX_DEGREE + 1] = {0};
  for (size_t i = 0; i < sm.size(); ++i) {
    if (!use[i]) continue;
    const double t = lmc_t(sm[i].xb, cols);
    double pw = 1.0;
    for (int k = 0; k <= 2 * degree; ++k) {
      M[k] = M[k] + pw;
      if (k < N) bv[k] = bv[k] + pw * sm[i].xs;
      pw = pw * t;
    }
  }
  double L[LM_CALIB_MAX_DEGREE + 1][LM_CALIB_MAX_DEGREE + 1] = {{0}};
  for (int j = 0; j < N; ++j) {
    double s = M[j + j];
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < N; ++i) {
      double v = M[i + j];
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[LM_CALIB_MAX_DEGREE + 1];
  for (int i = 0; i < N; ++i) {
    double v = bv[i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < N; ++k) v = v - L[k][i] * coef[k];
    coef[i] = v / L[i][i];
  }
  return true;
}

// Count and xb range of the flagged samples; the refusal's text, or empty.
inline std::string lmc_refusal(const std::vector<LmcSample>& sm, const std::vector<char>& use, int n_frames, int cols,
                               int degree, int* n_out, double* lo_out, double* hi_out) {
  int n = 0;
  double lo = 0, hi = 0;
  for (size_t i = 0; i < sm.size(); ++i) {
    if (!use[i]) continue;
    if (n == 0 || sm[i].xb < lo) lo = sm[i].xb;
    if (n == 0 || sm[i].xb > hi) hi = sm[i].xb;
    ++n;
  }
  *n_out = n;
  *lo_out = lo;
  *hi_out = hi;
  const int need = 8 * (degree + 1);
  if (n < need)
    return "calibration: " + std::to_string(n) + " samples of " + std::to_string(n_frames) + " frames; a fit of degree " +
           std::to_string(degree) + " needs at least " + std::to_string(need) + ".";
  if (hi - lo < (double)cols / 4.0)
    return "calibration: the samples cover columns " + std::to_string(lo) + " to " + std::to_string(hi) +
           "; the range must span at least " + std::to_string((double)cols / 4.0) + " (a quarter of the width).";
  return std::string();
}

// The fit; the refusal's text, or empty with *res filled.
inline std::string lmc_fit(const lm_calib_record* rec, int n_frames, int cols, const lm_calib_opts& o, int degree,
                           double max_resid, lm_calib_fit_result* res) {
  std::vector<LmcSample> sm;
  lmc_samples(rec, n_frames, o, sm);
  *res = lm_calib_fit_result{};
  res->n_frames = n_frames;
  res->n_samples = (int32_t)sm.size();
  res->degree = degree;
  std::vector<char> use(sm.size(), 1);
  double coef[LM_CALIB_MAX_DEGREE + 1] = {0};
  int n = 0;
  double lo = 0, hi = 0;
  for (int round = 0; round < 2; ++round) {
    std::string why = lmc_refusal(sm, use, n_frames, cols, degree, &n, &lo, &hi);
    if (!why.empty()) return why;
    if (!lmc_solve(sm, use, cols, degree, coef))
      return "calibration: the normal equations of the " + std::to_string(n) + " samples are not positive definite.";
    if (round == 0)
      for (size_t i = 0; i < sm.size(); ++i) {
        const double r = sm[i].xs - lmc_poly(coef, degree, lmc_t(sm[i].xb, cols));
        if (fabs(r) > max_resid) use[i] = 0;
      }
  }
  double ss = 0.0, worst = 0.0;
  for (size_t i = 0; i < sm.size(); ++i) {
    if (!use[i]) continue;
    const double r = sm[i].xs - lmc_poly(coef, degree, lmc_t(sm[i].xb, cols));
    ss = ss + r * r;
    if (fabs(r) > worst) worst = fabs(r);
  }
  res->n_used = n;
  res->rms = sqrt(ss / (double)n);
  res->max_abs_resid = worst;
  res->lo = lo;
  res->hi = hi;
  for (int k = 0; k <= degree; ++k) res->coef[k] = coef[k];
  return std::string();
}

// q(c): p on [lo, hi], continued linearly with p' at the nearer end outside.
inline double lmc_warp(const lm_calib_fit_result& f, int cols, double c) {
  const double half = (double)cols / 2.0;
  if (c < f.lo) {
    const double t = lmc_t(f.lo, cols);
    return lmc_poly(f.coef, f.degree, t) + lmc_poly_dt(f.coef, f.degree, t) / half * (c - f.lo);
  }
  if (c > f.hi) {
    const double t = lmc_t(f.hi, cols);
    return lmc_poly(f.coef, f.degree, t) + lmc_poly_dt(f.coef, f.degree, t) / half * (c - f.hi);
  }
  return lmc_poly(f.coef, f.degree, lmc_t(c, cols));
}

// m(c) for every column; the refusal's text when it is not non-decreasing.
inline std::string lmc_columns(const lm_calib_fit_result& f, int cols, std::vector<int32_t>& m) {
  m.resize((size_t)cols);
  for (int c = 0; c < cols; ++c) {
    double v = floor(lmc_warp(f, cols, (double)c) + 0.5);
    if (!(v >= 0.0)) v = 0.0;
    if (v > (double)(cols - 1)) v = (double)(cols - 1);
    m[(size_t)c] = (int32_t)v;
    if (c > 0 && m[(size_t)c] < m[(size_t)c - 1])
      return "calibration: the fitted warp is not non-decreasing: column " + std::to_string(c) + " maps to " +
             std::to_string(m[(size_t)c]) + " after " + std::to_string(m[(size_t)c - 1]) + ".";
  }
  return std::string();
}

inline std::string lmc_map(const lm_calib_fit_result& f, int rows, int cols, int split_row, int32_t* map, int32_t* boxes) {
  std::vector<int32_t> m;
  std::string why = lmc_columns(f, cols, m);
  if (!why.empty()) return why;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) map[(size_t)r * cols + c] = r * cols + (r < split_row ? m[(size_t)c] : c);
  const int32_t b[8] = {0, 0, cols, split_row, 0, split_row, cols, rows - split_row};
  for (int k = 0; k < 8; ++k) boxes[k] = b[k];
  return std::string();
}

#endif  // LM_CALIB_CORE_H
