// lm_train_core.h — the detector training's arithmetic (include/locomouse_train.h),
// compiled for host and device: a sample's part of the objective, of its
// gradient and of the line search, and the host statement of the whole (CPU
// tests; the kernels of lm_train.hip compute the same sums in their own fixed
// order).  Doubles only.
//
//   F(w, b) = 1/2 (|w|^2 + b^2) + sum_i C_{y_i} max(0, 1 - y_i z_i)^2,   z_i = w . x_i + b,  x_i = p_i / 255
//
// The matrix products run over the u8 patches p_i as they are stored (the
// conversion u8 -> double is exact) and are divided by 255 once per sum:
// z_i = (w . p_i) / 255 + b,  (X^T t)_j = (sum_i t_i p_ij) / 255.
//
// A sample matrix is N rows of D = kh * kw bytes, lmt_pitch(D) bytes apart,
// the bytes past D zero.
#ifndef LM_TRAIN_CORE_H
#define LM_TRAIN_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LMT_HD __host__ __device__ inline
#else
#define LMT_HD inline
#endif

#define LMT_LS_STEPS 24       // line search: lambda = 2^-k, k = 0 .. LMT_LS_STEPS - 1
#define LMT_ARMIJO 1e-4       // F(w + lambda d) - F(w) <= LMT_ARMIJO lambda g . d
#define LMT_CG_TOL 1e-3       // CG stops at |r| <= LMT_CG_TOL |g|
#define LMT_XT_BLOCK 1024     // samples per block of the X^T u pass (lm_train.hip's k_train_xt)

LMT_HD int lmt_pitch(int D) { return (D + 15) / 16 * 16; }

// Sample i at margin z: its cost a = C_{y} when it is active (y z < 1), else 0;
// *t = a (z - y), its coefficient in grad F = (w, b) + 2 X~^T t (y^2 = 1);
// *loss = a (1 - y z)^2.
LMT_HD double lmt_coef(int y, double z, double c_pos, double c_neg, double* t, double* loss) {
  const double yd = (double)y;
  const double m = 1.0 - yd * z;
  const double a = m > 0.0 ? (y > 0 ? c_pos : c_neg) : 0.0;
  *t = a * (z - yd);
  *loss = a * (m * m);
  return a;
}

// The cost C_i of a sample with label y in group `group` for a problem of
// lm_train_solve_many with costs c_pos, c_neg that holds group `held_out` out
// (-1: none): 0 for a held-out sample, else the cost of its label.  Handed to
// lmt_coef and lmt_ls_delta as both costs, a held-out sample's terms are +-0.
LMT_HD double lmt_problem_cost(int y, int group, double c_pos, double c_neg, int held_out) {
  return group == held_out ? 0.0 : (y > 0 ? c_pos : c_neg);
}

// Problems that share one pass over the matrix (lm_train.hip's k_train_xv and
// k_train_xt) at D = kh * kw: their vectors, lmt_pitch(D) + 1 doubles each, fit
// into LMT_MANY_LDS bytes of LDS, so that three workgroups share a CU's
// 160 KiB; at most LMT_MANY_PB, which the 16 column sums per problem of
// k_train_xt allow in registers.
#define LMT_MANY_PB 4
#define LMT_MANY_LDS (48 * 1024)
LMT_HD int lmt_problem_block(int D) {
  const int bytes = 8 * ((D + 15) / 16 * 16 + 1);
  int pb = LMT_MANY_PB;
  while (pb > 1 && pb * bytes > LMT_MANY_LDS) pb >>= 1;
  return pb;
}

// The solver's arrays of one problem (lm_train.hip) for N samples and vectors
// of VL doubles, in elements: the size of each, which is also the distance
// between consecutive problems' arrays in a call's allocation.
#define LMT_SAMPLE_BLOCK 256  // samples per workgroup of the per-sample kernels
#define LMT_N_VEC 6           // vectors: w, g, d, r, p, hp
#define LMT_N_SMP 5           // sample arrays: z, u, a, t, au
struct LmtLayout {
  int64_t nb, nblk;  // blocks of LMT_SAMPLE_BLOCK and of LMT_XT_BLOCK samples
  int64_t vec;       // LMT_N_VEC x VL
  int64_t smp;       // LMT_N_SMP x N
  int64_t part;      // part_loss, part_act (nb each), then lspart (nb x LMT_LS_STEPS)
  int64_t xtp;       // the X^T pass' block sums, nblk x VL
  int64_t counts;    // the held-out counts, nb x 4 (int32)
};
LMT_HD LmtLayout lmt_layout(int64_t N, int VL) {
  LmtLayout L;
  L.nb = (N + LMT_SAMPLE_BLOCK - 1) / LMT_SAMPLE_BLOCK;
  L.nblk = (N + LMT_XT_BLOCK - 1) / LMT_XT_BLOCK;
  L.vec = (int64_t)LMT_N_VEC * VL;
  L.smp = (int64_t)LMT_N_SMP * N;
  L.part = L.nb * (2 + LMT_LS_STEPS);
  L.xtp = L.nblk * VL;
  L.counts = L.nb * 4;
  return L;
}

// The change of sample i's loss when its margin goes from z to z + lambda xd.
LMT_HD double lmt_ls_delta(int y, double z, double xd, double lambda, double c_pos, double c_neg) {
  const double yd = (double)y, c = y > 0 ? c_pos : c_neg;
  double m0 = 1.0 - yd * z, m1 = 1.0 - yd * (z + lambda * xd);
  m0 = m0 > 0.0 ? m0 : 0.0;
  m1 = m1 > 0.0 ? m1 : 0.0;
  return c * ((m1 - m0) * (m1 + m0));
}

// ---- the host statement.  Vectors are D + 1 doubles: w, then b.

// z_i = (w . p_i) / 255 + b
inline void lmt_host_margins(const uint8_t* X, int64_t pitch, int64_t N, int D, const double* wb, double* z) {
  for (int64_t i = 0; i < N; ++i) {
    const uint8_t* p = X + i * pitch;
    double s = 0.0;
    for (int j = 0; j < D; ++j) s += wb[j] * (double)p[j];
    z[i] = s / 255.0 + wb[D];
  }
}

// out = X~^T t: out_j = (sum_i t_i p_ij) / 255, out_D = sum_i t_i
inline void lmt_host_xt(const uint8_t* X, int64_t pitch, int64_t N, int D, const double* t, double* out) {
  for (int j = 0; j <= D; ++j) out[j] = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    const uint8_t* p = X + i * pitch;
    for (int j = 0; j < D; ++j) out[j] += t[i] * (double)p[j];
    out[D] += t[i];
  }
  for (int j = 0; j < D; ++j) out[j] /= 255.0;
}

// F and grad F at wb; a (N doubles) gets the active costs.  Returns the number of active samples.
inline int64_t lmt_host_objective(const uint8_t* X, int64_t pitch, const int8_t* y, int64_t N, int D, double c_pos,
                                  double c_neg, const double* wb, double* z, double* a, double* t, double* F,
                                  double* grad) {
  lmt_host_margins(X, pitch, N, D, wb, z);
  double f = 0.0;
  int64_t n_active = 0;
  for (int64_t i = 0; i < N; ++i) {
    double loss;
    a[i] = lmt_coef(y[i], z[i], c_pos, c_neg, &t[i], &loss);
    f += loss;
    n_active += a[i] != 0.0;
  }
  double reg = 0.0;
  for (int j = 0; j <= D; ++j) reg += wb[j] * wb[j];
  *F = 0.5 * reg + f;
  lmt_host_xt(X, pitch, N, D, t, grad);
  for (int j = 0; j <= D; ++j) grad[j] = wb[j] + 2.0 * grad[j];
  return n_active;
}

// out = (I + 2 X~_A^T C_A X~_A) v with the active costs a; u, au: N doubles of scratch
inline void lmt_host_hessvec(const uint8_t* X, int64_t pitch, int64_t N, int D, const double* a, const double* v,
                             double* u, double* out) {
  lmt_host_margins(X, pitch, N, D, v, u);
  for (int64_t i = 0; i < N; ++i) u[i] *= a[i];
  lmt_host_xt(X, pitch, N, D, u, out);
  for (int j = 0; j <= D; ++j) out[j] = v[j] + 2.0 * out[j];
}

// Armijo backtracking from the cached margins z and xd = X~ d: the first
// lambda = 2^-k with F(wb + lambda d) - F(wb) <= LMT_ARMIJO lambda g.d, where
// wd = wb . d, dd = d . d, gd = g . d.  Returns k, or -1 when none of the
// LMT_LS_STEPS holds; *dF is the change of F at the step taken.
inline int lmt_host_linesearch(const int8_t* y, const double* z, const double* xd, int64_t N, double c_pos, double c_neg,
                               double wd, double dd, double gd, double* dF) {
  double lambda = 1.0;
  for (int k = 0; k < LMT_LS_STEPS; ++k, lambda *= 0.5) {
    double s = 0.0;
    for (int64_t i = 0; i < N; ++i) s += lmt_ls_delta(y[i], z[i], xd[i], lambda, c_pos, c_neg);
    const double d = lambda * wd + 0.5 * lambda * lambda * dd + s;
    if (d <= LMT_ARMIJO * lambda * gd) {
      *dF = d;
      return k;
    }
  }
  *dF = 0.0;
  return -1;
}

// ---- the same for a problem of lm_train_solve_many: group[i] is sample i's
// group, the samples of group held_out have cost 0 (lmt_problem_cost).  Their
// terms are +-0, which these sequential sums do not notice: the results equal,
// to the bit, those of the functions above on the samples that are left.

inline int64_t lmt_host_objective_heldout(const uint8_t* X, int64_t pitch, const int8_t* y, const uint8_t* group,
                                          int64_t N, int D, double c_pos, double c_neg, int held_out, const double* wb,
                                          double* z, double* a, double* t, double* F, double* grad) {
  lmt_host_margins(X, pitch, N, D, wb, z);
  double f = 0.0;
  int64_t n_active = 0;
  for (int64_t i = 0; i < N; ++i) {
    double loss;
    const double c = lmt_problem_cost(y[i], group[i], c_pos, c_neg, held_out);
    a[i] = lmt_coef(y[i], z[i], c, c, &t[i], &loss);
    f += loss;
    n_active += a[i] != 0.0;
  }
  double reg = 0.0;
  for (int j = 0; j <= D; ++j) reg += wb[j] * wb[j];
  *F = 0.5 * reg + f;
  lmt_host_xt(X, pitch, N, D, t, grad);
  for (int j = 0; j <= D; ++j) grad[j] = wb[j] + 2.0 * grad[j];
  return n_active;
}

inline int lmt_host_linesearch_heldout(const int8_t* y, const uint8_t* group, const double* z, const double* xd,
                                       int64_t N, double c_pos, double c_neg, int held_out, double wd, double dd,
                                       double gd, double* dF) {
  double lambda = 1.0;
  for (int k = 0; k < LMT_LS_STEPS; ++k, lambda *= 0.5) {
    double s = 0.0;
    for (int64_t i = 0; i < N; ++i) {
      const double c = lmt_problem_cost(y[i], group[i], c_pos, c_neg, held_out);
      s += lmt_ls_delta(y[i], z[i], xd[i], lambda, c, c);
    }
    const double d = lambda * wd + 0.5 * lambda * lambda * dd + s;
    if (d <= LMT_ARMIJO * lambda * gd) {
      *dF = d;
      return k;
    }
  }
  *dF = 0.0;
  return -1;
}

#endif  // LM_TRAIN_CORE_H
