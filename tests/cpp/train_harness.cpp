// train_harness.cpp — the host build of csrc/lm_train_core.h for ctypes
// (tests/train_harness.py; no GPU library): objective and gradient, the
// active-set Hessian product, the line search.
#include <cmath>
#include <cstdint>
#include <vector>

#include "lm_train_core.h"

extern "C" {

int th_pitch(int D) { return lmt_pitch(D); }
int th_ls_steps() { return LMT_LS_STEPS; }
int th_xt_block() { return LMT_XT_BLOCK; }

// F, grad (D + 1), the margins z and the active costs a (N each); returns the active count
int64_t th_objective(const uint8_t* X, int64_t pitch, const int8_t* y, int64_t N, int D, double c_pos, double c_neg,
                     const double* wb, double* z, double* a, double* F, double* grad) {
  std::vector<double> t((size_t)N);
  return lmt_host_objective(X, pitch, y, N, D, c_pos, c_neg, wb, z, a, t.data(), F, grad);
}

void th_hessvec(const uint8_t* X, int64_t pitch, int64_t N, int D, const double* a, const double* v, double* out) {
  std::vector<double> u((size_t)N);
  lmt_host_hessvec(X, pitch, N, D, a, v, u.data(), out);
}

void th_margins(const uint8_t* X, int64_t pitch, int64_t N, int D, const double* wb, double* z) {
  lmt_host_margins(X, pitch, N, D, wb, z);
}

int th_linesearch(const int8_t* y, const double* z, const double* xd, int64_t N, double c_pos, double c_neg, double wd,
                  double dd, double gd, double* dF) {
  return lmt_host_linesearch(y, z, xd, N, c_pos, c_neg, wd, dd, gd, dF);
}

// filter2D's fused fp32 chain over one patch (8U -> 32F): from (float)(-rho),
// the non-zero taps in row-major order, one fma each
float th_fused_score(const uint8_t* patch, const double* W, int D, double rho) {
  float acc = (float)(-rho);
  for (int j = 0; j < D; ++j) {
    const float w = (float)W[j];
    if (w == 0.0f) continue;
    acc = std::fmaf(w, (float)patch[j], acc);
  }
  return acc;
}

}  // extern "C"
