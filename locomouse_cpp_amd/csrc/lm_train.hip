// lm_train.hip — detector training (include/locomouse_train.h): the sample
// matrix in device memory as u8 (rows lmt_pitch(D) bytes apart, padding zero),
// the gather that cuts samples from frames as detection reads them, and a
// truncated Newton solver of the squared-hinge SVM in fp64 (lm_train_core.h).
//
// Vectors of the solver have VL = Dp + 1 doubles, Dp = lmt_pitch(D): the
// weights at 0 .. D-1, zeros up to Dp (the matrix' padding columns are zero,
// so they stay zero), the bias at Dp.
//
//   k_train_gather     one workgroup per point: its kh x kw taps through
//                      ipad_pixel (lm_dev_common.h), the read of k_ingest.
//
// One solver: lm_train_solve is a call of one problem, lm_train_solve_many of
// up to LM_TRAIN_MAX_PROBLEMS on the same samples, lm_train_margins one X~ v
// pass of one problem.  A problem is its costs and its held-out group; its
// arrays lie one after the other problem's (LmtLayout, lm_train_core.h).  The
// two matrix passes take a block of problems (lmt_problem_block) per workgroup
// and convert a chunk of the matrix once for all of them, the other kernels
// one problem per workgroup row.
//
//   k_train_xv         out = X~ v: L = 2^k lanes per sample (L >= D / 16, at
//                      most 64) and four consecutive samples per lane group,
//                      so 256 / L samples per wave; the problems' v in LDS; a
//                      lane loads 16 bytes of each of its samples' rows at a
//                      time; the L lanes' sums are folded by xor butterflies
//                      (the same pairs whatever the lane, so every lane has
//                      the sum).
//   k_train_xt         X^T t: a workgroup takes LMT_XT_BLOCK samples and 256
//                      columns; a thread owns 16 columns, accumulates them in
//                      registers over every 16th sample of the block, the 16
//                      sample lanes are added in lane order through LDS, and
//                      the block's sums go to partial[block][VL].
//   k_train_xt_reduce  adds the blocks in index order: out = base + 2 sum.
//   k_train_coef       per sample: active cost, gradient coefficient, loss.
//   k_train_eval       one workgroup: F, |grad F|, the convergence flag, and
//                      the start of CG (d = 0, r = p = -g).
//   k_train_cg_update  one workgroup: a CG step's scalars and vector updates.
//   k_train_ls_partials / k_train_ls_pick   the Armijo search over
//                      lambda = 2^-k from the cached margins, all k at once.
//   k_train_heldout    the held-out group's samples and misses of a problem.
//
// An outer iteration is enqueued whole: the CG steps (a fixed number of
// them, each a no-op once the residual is small) and the line search read
// their flags from the problem's control block in device memory, and the host
// reads the blocks once per outer iteration.  Every sum is taken in an order
// that depends on N and D alone: strided per-thread sums, then a binary tree
// in LDS; blocks of samples in index order.  No atomics.
//
// Safety: sample rows are read at i * Dp for i < N <= max_samples, which
// sizes the matrix; vectors have VL entries and are indexed below VL.  The
// gather writes rows n0 .. n0 + n_points - 1 with n0 + n_points <= max_samples,
// and its points' frame indices and coordinates are checked on the host; taps
// outside the corrected image read nothing.  The solver's kernels index a
// problem's arrays at q * stride with q < the call's problem count; strides
// and sizes are LmtLayout's for the N and VL of the call (bind_problems): the
// vectors V_W .. V_HP, the sample arrays S_Z .. S_AU, two nb-long parts and
// nb x LMT_LS_STEPS of lspart, nblk rows of block sums, nb x 4 counts; a block's
// slots past the last problem read the block's first problem and write nothing;
// the LDS of k_train_xv holds lmt_problem_block x VL doubles, at most 48 KiB
// (one vector, 32 KB, at 64 x 64); the group bytes are sized by max_samples.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "locomouse_train.h"
#include "lm_dev_common.h"
#include "lm_host.h"
#include "lm_train_core.h"

namespace {

constexpr int kT = 256;       // threads of every workgroup here
constexpr int kXvS = 4;       // samples per lane group of k_train_xv
constexpr int kXtCols = 256;  // columns per workgroup of k_train_xt (16 column groups of 16)

struct LmtCtl {  // the solver's scalars in device memory
  double f, gnorm, gnorm0, rr;
  int32_t converged, cg_done, cg_iters, n_active, ls_fail;
};
enum { GATE_NONE = 0, GATE_CG = 1, GATE_CONVERGED = 2 };

// Sum of v over the workgroup's kT threads, by a binary tree of fixed shape.
DEV double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// Sum of x[0 .. n): thread t adds x[t], x[t + kT], .. in that order, then the tree.
DEV double block_sum_array(const double* x, int n, double* sh) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += kT) a += x[i];
  return block_sum(a, sh);
}

__global__ __launch_bounds__(kT) void k_train_gather(const LmConst* __restrict__ Kp,
                                                     const uint8_t* const* __restrict__ frame_ptr,
                                                     const uint8_t* __restrict__ bkg, const int32_t* __restrict__ cal,
                                                     const uint8_t* __restrict__ luts,
                                                     const lm_train_point* __restrict__ pts, int kh, int kw, int Dp,
                                                     uint8_t* __restrict__ rows) {
  const LmConst& K = *Kp;
  const lm_train_point pt = pts[blockIdx.x];
  const lm_gu8* F = as_global(frame_ptr[pt.frame]);
  const uint8_t* lut = luts + (int64_t)pt.frame * 256;
  uint8_t* dst = rows + (int64_t)blockIdx.x * Dp;
  const int D = kh * kw;
  for (int e = threadIdx.x; e < Dp; e += kT) {
    uint8_t v = 0;
    if (e < D) {
      const int i = e / kw, j = e - i * kw;
      v = ipad_pixel(F, bkg, cal, lut, K, K.pad_pre_rows + pt.y - kh / 2 + i, K.pad_pre_cols + pt.x - kw / 2 + j);
    }
    dst[e] = v;
  }
}

// ---- the solver, for the problems of a call on the same samples.  A problem
// is its costs, its held-out group and its own LmtCtl; its arrays lie `stride`
// doubles after its predecessor's (lm_train_core.h's LmtLayout).  The two
// matrix passes take a block of pb problems (lmt_problem_block) per workgroup,
// block b of the call along a grid dimension, and load and convert a 16-byte
// chunk once for those of them that are live; the other kernels take one
// problem per workgroup row.  Per problem every sum is the same, term for
// term, whatever the company.  A problem that is done (converged, or without
// a line-search step) is gated everywhere, the evaluation included, so its
// arrays stay as a call of it alone leaves them when the host stops; a
// workgroup whose problems are all gated returns at once, and one with fewer
// live problems than pb computes for 1, 2 or 4 of them.

struct LmtProb {  // a problem in device memory
  double c_pos, c_neg;
  int32_t held_out, pad;
};

struct LmtProblems {
  int n;  // problems of the call
  const LmtProb* prob;
  LmtCtl* ctl;
  const uint8_t* group;  // per sample
  double* vec;           // per problem w, g, d, r, p, hp: 6 x VL
  double* smp;           // per problem z, u, a, t, au: 5 x N
  double* part;          // per problem part_loss, part_act (nb each), lspart (nb x LMT_LS_STEPS)
  double* xtp;           // per problem nblk x VL
  int64_t vec_stride, smp_stride, part_stride, xtp_stride;
};
enum { V_W = 0, V_G, V_D, V_R, V_P, V_HP };
enum { S_Z = 0, S_U, S_A, S_T, S_AU, S_NONE = -1 };
static_assert(V_HP + 1 == LMT_N_VEC && S_AU + 1 == LMT_N_SMP && kT == LMT_SAMPLE_BLOCK, "LmtLayout sizes these");

DEV bool gated(const LmtCtl* ctl, int gate) {
  return (gate == GATE_CG && (ctl->cg_done || ctl->ls_fail)) || (gate == GATE_CONVERGED && (ctl->converged || ctl->ls_fail));
}

// The live problems of q0 .. q0 + pb - 1 (those that exist and are not gated),
// in their order: q[j] is the j-th, q[j] = q[0] from their number on, which is
// returned.  (Unrolled selects: the list stays in scalar registers.)
struct LmtLive {
  int q[LMT_MANY_PB];
};
DEV int live_problems(const LmtProblems& M, int q0, int pb, int gate, LmtLive& live) {
  int nl = 0;
#pragma unroll
  for (int j = 0; j < LMT_MANY_PB; ++j) live.q[j] = q0;
#pragma unroll
  for (int p = 0; p < LMT_MANY_PB; ++p) {
    if (p < pb && q0 + p < M.n && !gated(M.ctl + q0 + p, gate)) {
#pragma unroll
      for (int j = 0; j < LMT_MANY_PB; ++j) live.q[j] = j == nl ? q0 + p : live.q[j];
      nl += 1;
    }
  }
#pragma unroll
  for (int j = 1; j < LMT_MANY_PB; ++j) live.q[j] = j < nl ? live.q[j] : live.q[0];
  return nl;
}

// k_train_xv with NP slots: slot p is live problem p (a slot past the nl live
// ones computes on the first one's vector and writes nothing).  Entry 16 g + k
// of slot p's vector is at sv[(k * ncg + g) * NP + p] (lanes of consecutive
// chunks g read consecutive words), its bias at sv[Dp * NP + p].
template <int NP>
DEV void xv_slots(const uint8_t* __restrict__ X, int64_t N, int Dp, int L, const LmtProblems& M, const LmtLive& live, int nl,
                 int vi, double div, int ai, int oi, int oai, double* sv) {
  const int ncg = Dp >> 4, VL = Dp + 1;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const double* v = M.vec + (int64_t)live.q[p] * M.vec_stride + (int64_t)vi * VL;
    for (int j = threadIdx.x; j < Dp; j += kT) sv[((j & 15) * ncg + (j >> 4)) * NP + p] = v[j];
    if (threadIdx.x == 0) sv[Dp * NP + p] = v[Dp];
  }
  __syncthreads();
  const int gl = threadIdx.x & (L - 1);
  const int64_t i0 = ((int64_t)blockIdx.x * (kT / L) + threadIdx.x / L) * kXvS;
  double acc[NP][kXvS];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int s = 0; s < kXvS; ++s) acc[p][s] = 0.0;
  for (int g = gl; g < ncg; g += L) {
    uint4 q[kXvS];
#pragma unroll
    for (int s = 0; s < kXvS; ++s)
      q[s] = i0 + s < N ? reinterpret_cast<const uint4*>(X + (i0 + s) * Dp)[g] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double* w = sv + (k * ncg + g) * NP;
      double wk[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) wk[p] = w[p];
#pragma unroll
      for (int s = 0; s < kXvS; ++s) {
        const uint32_t word = (k >> 2) == 0 ? q[s].x : (k >> 2) == 1 ? q[s].y : (k >> 2) == 2 ? q[s].z : q[s].w;
        const double x = (double)((word >> (8 * (k & 3))) & 255u);  // once for the NP problems
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p][s] += x * wk[p];
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    double* smp = M.smp + (int64_t)live.q[p] * M.smp_stride;
    const double bias = sv[Dp * NP + p];
#pragma unroll
    for (int s = 0; s < kXvS; ++s) {
      double r = acc[p][s];
      for (int o = L >> 1; o > 0; o >>= 1) r += __shfl_xor(r, o);
      if (gl == 0 && i0 + s < N && p < nl) {
        const double z = r / div + bias;
        smp[(int64_t)oi * N + i0 + s] = z;
        if (ai != S_NONE) smp[(int64_t)oai * N + i0 + s] = smp[(int64_t)ai * N + i0 + s] * z;
      }
    }
  }
}

// Sample array oi = X~ (vector vi) of the problems q0 .. q0 + pb - 1, q0 = pb
// blockIdx.y; with ai, sample array oai = sample array ai times it.
__global__ __launch_bounds__(kT) void k_train_xv(const uint8_t* __restrict__ X, int64_t N, int Dp, int L, LmtProblems M,
                                                      int pb, int vi, double div, int ai, int oi, int oai, int gate) {
  LmtLive live;
  const int nl = live_problems(M, blockIdx.y * pb, pb, gate, live);
  if (nl == 0) return;
  extern __shared__ double sv[];  // pb x VL doubles
  if (nl == 1)
    xv_slots<1>(X, N, Dp, L, M, live, nl, vi, div, ai, oi, oai, sv);
  else if (nl == 2)
    xv_slots<2>(X, N, Dp, L, M, live, nl, vi, div, ai, oi, oai, sv);
  else
    xv_slots<4>(X, N, Dp, L, M, live, nl, vi, div, ai, oi, oai, sv);
}

// k_train_xt with NP slots (as xv_slots'): the block's sums of X^T t of each,
// t = the problem's sample array ti.  A chunk is loaded and converted once;
// the 16 sample lanes are added through LDS one problem after the other.
template <int NP>
DEV void xt_slots(const uint8_t* __restrict__ X, int64_t N, int Dp, const LmtProblems& M, const LmtLive& live, int nl, int ti,
                 double (*red)[kXtCols], double* redb) {
  const int cgx = threadIdx.x & 15, sy = threadIdx.x >> 4;
  const int g = blockIdx.x * 16 + cgx;  // column group of 16
  const bool cols = g < (Dp >> 4);
  const bool bias = blockIdx.x == 0 && cgx == 0;
  const int64_t i0 = (int64_t)blockIdx.y * LMT_XT_BLOCK;
  const int64_t i1 = i0 + LMT_XT_BLOCK < N ? i0 + LMT_XT_BLOCK : N;
  const double* t[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) t[p] = M.smp + (int64_t)live.q[p] * M.smp_stride + (int64_t)ti * N;
  double acc[NP][16], tb[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    tb[p] = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[p][k] = 0.0;
  }
  if (cols || bias) {
    for (int64_t i = i0 + sy; i < i1; i += 16) {
      double tv[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) tv[p] = t[p][i];
      if (bias) {
#pragma unroll
        for (int p = 0; p < NP; ++p) tb[p] += tv[p];
      }
      if (cols) {
        const uint4 q = *reinterpret_cast<const uint4*>(X + i * Dp + 16 * g);
        const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const double x = (double)((word[k >> 2] >> (8 * (k & 3))) & 255u);  // once for the NP problems
#pragma unroll
          for (int p = 0; p < NP; ++p) acc[p][k] += tv[p] * x;
        }
      }
    }
  }
  const int VL = Dp + 1;
  const int c = blockIdx.x * kXtCols + threadIdx.x;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (p >= nl) break;          // (uniform)
    if (p > 0) __syncthreads();  // red is read no more
#pragma unroll
    for (int k = 0; k < 16; ++k) red[sy][cgx * 16 + k] = acc[p][k];
    if (bias) redb[sy] = tb[p];
    __syncthreads();
    double* prow = M.xtp + (int64_t)live.q[p] * M.xtp_stride + (int64_t)blockIdx.y * VL;
    if (c < Dp) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += red[q][threadIdx.x];
      prow[c] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      double s = 0.0;
      for (int q = 0; q < 16; ++q) s += redb[q];
      prow[Dp] = s;
    }
  }
}

// The blocks' sums of X^T (sample array ti) of the problems q0 .. q0 + pb - 1, q0 = pb blockIdx.z.
__global__ __launch_bounds__(kT) void k_train_xt(const uint8_t* __restrict__ X, int64_t N, int Dp, LmtProblems M, int pb,
                                                      int ti, int gate) {
  LmtLive live;
  const int nl = live_problems(M, blockIdx.z * pb, pb, gate, live);
  if (nl == 0) return;
  __shared__ double red[16][kXtCols];
  __shared__ double redb[16];
  if (nl == 1)
    xt_slots<1>(X, N, Dp, M, live, nl, ti, red, redb);
  else if (nl == 2)
    xt_slots<2>(X, N, Dp, M, live, nl, ti, red, redb);
  else
    xt_slots<4>(X, N, Dp, M, live, nl, ti, red, redb);
}

// From here on blockIdx.y is the problem.

// vector oi = vector bi + 2 X~^T t from the blocks' sums, in index order
__global__ __launch_bounds__(kT) void k_train_xt_reduce(LmtProblems M, int nblk, int Dp, int bi, int oi, int gate) {
  const int q = blockIdx.y;
  if (gated(M.ctl + q, gate)) return;
  const int VL = Dp + 1;
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= VL) return;
  const double* partial = M.xtp + (int64_t)q * M.xtp_stride;
  double* vec = M.vec + (int64_t)q * M.vec_stride;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * VL + j];
  if (j < Dp) s = s / 255.0;
  vec[(int64_t)oi * VL + j] = vec[(int64_t)bi * VL + j] + 2.0 * s;
}

// Per sample: its cost (none for a held-out one), active cost, gradient coefficient and loss; the block's sums.
__global__ __launch_bounds__(kT) void k_train_coef(LmtProblems M, const int8_t* __restrict__ y, int64_t N, int nb) {
  const int q = blockIdx.y;
  if (gated(M.ctl + q, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
  const LmtProb pr = M.prob[q];
  double* smp = M.smp + (int64_t)q * M.smp_stride;
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  double loss = 0.0, act = 0.0;
  if (i < N) {
    double ti;
    const double c = lmt_problem_cost(y[i], M.group[i], pr.c_pos, pr.c_neg, pr.held_out);
    const double ai = lmt_coef(y[i], smp[(int64_t)S_Z * N + i], c, c, &ti, &loss);
    smp[(int64_t)S_A * N + i] = ai;
    smp[(int64_t)S_T * N + i] = ti;
    act = ai != 0.0 ? 1.0 : 0.0;
  }
  const double sl = block_sum(loss, sh);
  const double sa = block_sum(act, sh);  // (counts below 2^53 are exact in a double)
  if (threadIdx.x == 0) {
    double* part = M.part + (int64_t)q * M.part_stride;
    part[blockIdx.x] = sl;
    part[nb + blockIdx.x] = sa;
  }
}

// F and |grad F| at w from the parts; sets the flags; d = 0, r = p = -g.
__global__ __launch_bounds__(kT) void k_train_eval(LmtProblems M, int VL, int nb, double eps, int first) {
  const int q = blockIdx.x;
  LmtCtl* ctl = M.ctl + q;
  if (gated(ctl, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
  double* vec = M.vec + (int64_t)q * M.vec_stride;
  const double *w = vec + (int64_t)V_W * VL, *g = vec + (int64_t)V_G * VL;
  double *d = vec + (int64_t)V_D * VL, *r = vec + (int64_t)V_R * VL, *p = vec + (int64_t)V_P * VL;
  const double* part = M.part + (int64_t)q * M.part_stride;
  double ww = 0.0, gg = 0.0;
  for (int j = threadIdx.x; j < VL; j += kT) {
    ww += w[j] * w[j];
    gg += g[j] * g[j];
    d[j] = 0.0;
    r[j] = -g[j];
    p[j] = -g[j];
  }
  ww = block_sum(ww, sh);
  gg = block_sum(gg, sh);
  const double loss = block_sum_array(part, nb, sh);
  const double act = block_sum_array(part + nb, nb, sh);
  if (threadIdx.x == 0) {
    const double gnorm = sqrt(gg);
    const double g0 = first ? gnorm : ctl->gnorm0;
    ctl->f = 0.5 * ww + loss;
    ctl->gnorm = gnorm;
    ctl->gnorm0 = g0;
    ctl->rr = gg;
    ctl->n_active = (int32_t)act;
    ctl->converged = gnorm <= eps * g0 ? 1 : 0;
    ctl->cg_done = ctl->converged;
  }
}

// One CG step on (I + 2 X~_A^T C_A X~_A) d = -g with hp = H p already computed.
__global__ __launch_bounds__(kT) void k_train_cg_update(LmtProblems M, int VL) {
  const int q = blockIdx.x;
  LmtCtl* ctl = M.ctl + q;
  if (gated(ctl, GATE_CG)) return;
  __shared__ double sh[kT];
  double* vec = M.vec + (int64_t)q * M.vec_stride;
  double *d = vec + (int64_t)V_D * VL, *r = vec + (int64_t)V_R * VL, *p = vec + (int64_t)V_P * VL;
  const double* hp = vec + (int64_t)V_HP * VL;
  const double rr = ctl->rr, gnorm = ctl->gnorm;
  double a = 0.0;
  for (int j = threadIdx.x; j < VL; j += kT) a += p[j] * hp[j];
  const double php = block_sum(a, sh);  // >= |p|^2 > 0: H - I is positive semi-definite and r != 0
  const double alpha = rr / php;
  double b = 0.0;
  for (int j = threadIdx.x; j < VL; j += kT) {
    d[j] += alpha * p[j];
    const double rj = r[j] - alpha * hp[j];
    r[j] = rj;
    b += rj * rj;
  }
  const double rr1 = block_sum(b, sh);
  const double beta = rr1 / rr;
  for (int j = threadIdx.x; j < VL; j += kT) p[j] = r[j] + beta * p[j];
  if (threadIdx.x == 0) {
    ctl->rr = rr1;
    ctl->cg_iters += 1;
    if (!(sqrt(rr1) > LMT_CG_TOL * gnorm)) ctl->cg_done = 1;
  }
}

// Per block of kT samples, the change of their losses at every lambda = 2^-k.
__global__ __launch_bounds__(kT) void k_train_ls_partials(LmtProblems M, const int8_t* __restrict__ y, int64_t N,
                                                               int nb) {
  const int q = blockIdx.y;
  if (gated(M.ctl + q, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
  const LmtProb pr = M.prob[q];
  const double* smp = M.smp + (int64_t)q * M.smp_stride;
  double* lspart = M.part + (int64_t)q * M.part_stride + 2 * (int64_t)nb;
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = i < N;
  const int yi = valid ? y[i] : 1;
  const double c = valid ? lmt_problem_cost(yi, M.group[i], pr.c_pos, pr.c_neg, pr.held_out) : 0.0;
  const double zi = valid ? smp[(int64_t)S_Z * N + i] : 0.0, xi = valid ? smp[(int64_t)S_U * N + i] : 0.0;
  double lambda = 1.0;
  for (int k = 0; k < LMT_LS_STEPS; ++k, lambda *= 0.5) {
    const double v = valid ? lmt_ls_delta(yi, zi, xi, lambda, c, c) : 0.0;
    const double s = block_sum(v, sh);
    if (threadIdx.x == 0) lspart[(int64_t)blockIdx.x * LMT_LS_STEPS + k] = s;
  }
}

// The first lambda that satisfies Armijo; w += lambda d.
__global__ __launch_bounds__(kT) void k_train_ls_pick(LmtProblems M, int VL, int nb) {
  const int q = blockIdx.x;
  LmtCtl* ctl = M.ctl + q;
  if (gated(ctl, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
  double* vec = M.vec + (int64_t)q * M.vec_stride;
  double* w = vec + (int64_t)V_W * VL;
  const double *g = vec + (int64_t)V_G * VL, *d = vec + (int64_t)V_D * VL;
  const double* lspart = M.part + (int64_t)q * M.part_stride + 2 * (int64_t)nb;
  double wd = 0.0, dd = 0.0, gd = 0.0;
  for (int j = threadIdx.x; j < VL; j += kT) {
    wd += w[j] * d[j];
    dd += d[j] * d[j];
    gd += g[j] * d[j];
  }
  wd = block_sum(wd, sh);
  dd = block_sum(dd, sh);
  gd = block_sum(gd, sh);
  int picked = -1;  // (uniform: every thread sees the same sums)
  double lambda = 1.0, step = 0.0;
  for (int k = 0; k < LMT_LS_STEPS; ++k, lambda *= 0.5) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += kT) a += lspart[(int64_t)b * LMT_LS_STEPS + k];
    const double s = block_sum(a, sh);
    const double delta = lambda * wd + 0.5 * lambda * lambda * dd + s;
    if (picked < 0 && delta <= LMT_ARMIJO * lambda * gd) {
      picked = k;
      step = lambda;
    }
  }
  if (picked >= 0)
    for (int j = threadIdx.x; j < VL; j += kT) w[j] += step * d[j];
  if (threadIdx.x == 0 && picked < 0) ctl->ls_fail = 1;
}

// Per block of kT samples and problem, the held-out group's samples by label
// and those on the wrong side of z, the margins of the last evaluation:
// counts[(q * nb + block) * 4 + (n_pos, n_neg, miss_pos, miss_neg)].
__global__ __launch_bounds__(kT) void k_train_heldout(LmtProblems M, const int8_t* __restrict__ y, int64_t N, int nb,
                                                      int32_t* __restrict__ counts) {
  const int q = blockIdx.y;
  __shared__ int32_t sh[4][kT];
  const int held_out = M.prob[q].held_out;
  const double* z = M.smp + (int64_t)q * M.smp_stride + (int64_t)S_Z * N;
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  int32_t v[4] = {0, 0, 0, 0};
  if (i < N && (int)M.group[i] == held_out) {
    const bool pos = y[i] > 0, above = z[i] > 0.0;
    v[0] = pos;
    v[1] = !pos;
    v[2] = pos && !above;
    v[3] = !pos && above;
  }
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sh[k][t] += sh[k][t + s];
    }
    __syncthreads();
  }
  if (t < 4) counts[((int64_t)q * nb + blockIdx.x) * 4 + t] = sh[t][0];
}

}  // namespace

struct lm_train_ctx {
  int device = 0;
  int kh = 0, kw = 0, D = 0, Dp = 0, VL = 0;
  int64_t max_samples = 0, n = 0;
  int64_t n_pos = 0;
  hipStream_t stream = nullptr;
  DevBuf<uint8_t> X;
  DevBuf<int8_t> y;
  std::vector<int8_t> h_y;
  // groups (lm_train_set_groups)
  bool groups_set = false;
  std::vector<uint8_t> h_group;
  DevBuf<uint8_t> group;  // max_samples; all 0 while no groups are set (no problem holds a group out then)
  // solver: the arrays of a call's problems (LmtProblems), sized per call by bind_problems
  DevBuf<double> vec, smp, part, xtp;
  DevBuf<int32_t> counts;
  DevBuf<LmtProb> prob;   // LM_TRAIN_MAX_PROBLEMS, as ctl and h_ctl
  DevBuf<LmtCtl> ctl;
  HostBuf<LmtCtl> h_ctl;
  // gather
  DevBuf<uint8_t> stage, luts;
  DevBuf<unsigned> mm;
  DevBuf<const uint8_t*> frame_ptr;
  DevBuf<lm_train_point> pts;
  ~lm_train_ctx() {
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

int lanes_per_sample(int Dp) {
  const int ncg = Dp >> 4;
  int L = 1;
  while (L < ncg && L < 64) L <<= 1;
  return L;
}

void check_add(const lm_train_ctx* c, int64_t n) {
  if (n < 0) throw std::invalid_argument("n is negative");
  if (c->n + n > c->max_samples)
    throw std::invalid_argument("the add would pass max_samples (" + std::to_string(c->max_samples) + "): " +
                                std::to_string(c->n) + " + " + std::to_string(n));
}

void commit_labels(lm_train_ctx* c, const int8_t* labels, int64_t n) {
  COPY_SYNC(c->y.p + c->n, labels, (size_t)n, hipMemcpyHostToDevice, c->stream);
  for (int64_t i = 0; i < n; ++i) c->n_pos += labels[i] > 0;
  c->h_y.insert(c->h_y.end(), labels, labels + n);
  c->n += n;
  c->groups_set = false;
}

lm_status gather(lm_train_ctx* c, lm_ctx* det, const uint8_t* frames, int64_t pitch, int32_t n_frames,
                 const lm_train_point* points, int32_t n_points, bool device_frames) {
  if (!c || !det || !frames || (!points && n_points > 0)) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    LmTrainView V;
    lm_ctx_train_view(det, &V);
    if (V.device != c->device) throw std::invalid_argument("the detection context is on another device");
    if (V.gray_lut_on)
      throw std::invalid_argument("transform_gray_values: that table moves with the per-frame crop; not gathered");
    if (V.matched)
      throw std::invalid_argument("a matched context (lm_ctx_create_matched): the table is the frame's own and moves with "
                                  "the per-frame crop; not gathered");
    if (n_frames <= 0 || n_frames > 65535) throw std::invalid_argument("n_frames must be in 1..65535");
    if (pitch < V.npix) throw std::invalid_argument("pitch is smaller than a frame");
    check_add(c, n_points);
    std::vector<int8_t> labels((size_t)(n_points > 0 ? n_points : 0));
    for (int32_t k = 0; k < n_points; ++k) {
      const lm_train_point& p = points[k];
      if (p.frame < 0 || p.frame >= n_frames)
        throw std::invalid_argument("point " + std::to_string(k) + ": frame index " + std::to_string(p.frame) +
                                    " is outside the call's " + std::to_string(n_frames) + " frames");
      if (p.x < 0 || p.x >= V.n_cols || p.y < 0 || p.y >= V.n_rows)
        throw std::invalid_argument("point " + std::to_string(k) + ": (" + std::to_string(p.x) + ", " +
                                    std::to_string(p.y) + ") is outside the corrected image");
      if (p.label != 1 && p.label != -1)
        throw std::invalid_argument("point " + std::to_string(k) + ": label must be +1 or -1");
      labels[(size_t)k] = (int8_t)p.label;
    }
    if (n_points == 0) return;
    HIPCHK(hipSetDevice(c->device));
    // the frames, 16-byte aligned in this context's memory (k_minmax loads 16 bytes per lane)
    const size_t fstride = ((size_t)V.npix + 15) / 16 * 16;
    if (c->stage.n < fstride * (size_t)n_frames) c->stage.alloc(fstride * (size_t)n_frames);
    if (c->luts.n < 256 * (size_t)n_frames) {
      c->luts.alloc(256 * (size_t)n_frames);
      c->mm.alloc(2 * LM_MM_SPLIT * (size_t)n_frames);
      c->frame_ptr.alloc((size_t)n_frames);
    }
    if (c->pts.n < (size_t)n_points) c->pts.alloc((size_t)n_points);
    HIPCHK(hipMemcpy2DAsync(c->stage.p, fstride, frames, (size_t)pitch, (size_t)V.npix, (size_t)n_frames,
                            device_frames ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    std::vector<const uint8_t*> fp((size_t)n_frames);
    for (int32_t i = 0; i < n_frames; ++i) fp[(size_t)i] = c->stage.p + (size_t)i * fstride;
    HIPCHK(hipMemcpyAsync(c->frame_ptr.p, fp.data(), sizeof(fp[0]) * fp.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->pts.p, points, sizeof(lm_train_point) * (size_t)n_points, hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // fp and the caller's arrays are free again
    HIPCHK(launch_minmax_lut(c->frame_ptr.p, V.bkg, V.npix, 0, n_frames, c->mm.p, V.adj, V.use_adj, c->luts.p,
                             c->stream));
    hipLaunchKernelGGL(k_train_gather, dim3((unsigned)n_points), dim3(kT), 0, c->stream, (const LmConst*)V.dK,
                       c->frame_ptr.p, V.bkg, V.cal, c->luts.p, c->pts.p, c->kh, c->kw, c->Dp,
                       c->X.p + (size_t)c->n * (size_t)c->Dp);
    HIPCHK(hipGetLastError());
    commit_labels(c, labels.data(), n_points);  // (waits for the stream)
  });
}

}  // namespace

LM_API lm_status lm_train_create(int32_t device, int32_t kh, int32_t kw, int32_t max_samples, lm_train_ctx** out) {
  if (!out) return fail(LM_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (kh < 1 || kh > LM_TRAIN_MAX_SIDE || kw < 1 || kw > LM_TRAIN_MAX_SIDE)
    return fail(LM_ERR_INVALID_ARGUMENT, "kh and kw must be in 1..64");
  if (max_samples < 1 || max_samples > LM_TRAIN_MAX_SAMPLES)
    return fail(LM_ERR_INVALID_ARGUMENT, "max_samples must be in 1..2^22");
  lm_train_ctx* c = new lm_train_ctx();
  lm_status s = guarded([&] {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw HipError("invalid HIP device index");
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->kh = kh;
    c->kw = kw;
    c->D = kh * kw;
    c->Dp = lmt_pitch(c->D);
    c->VL = c->Dp + 1;
    c->max_samples = max_samples;
    c->X.alloc((size_t)max_samples * (size_t)c->Dp);
    c->y.alloc((size_t)max_samples);
  });
  if (s != LM_OK) {
    delete c;
    return s;
  }
  *out = c;
  return LM_OK;
}

LM_API void lm_train_destroy(lm_train_ctx* ctx) { delete ctx; }

LM_API lm_status lm_train_add_patches(lm_train_ctx* ctx, const uint8_t* patches, const int8_t* labels, int32_t n) {
  if (!ctx || ((!patches || !labels) && n > 0)) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_add(ctx, n);
    for (int32_t i = 0; i < n; ++i)
      if (labels[i] != 1 && labels[i] != -1)
        throw std::invalid_argument("label " + std::to_string(i) + " is " + std::to_string((int)labels[i]) +
                                    ": must be +1 or -1");
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t* dst = ctx->X.p + (size_t)ctx->n * (size_t)ctx->Dp;
    HIPCHK(hipMemsetAsync(dst, 0, (size_t)n * (size_t)ctx->Dp, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)ctx->Dp, patches, (size_t)ctx->D, (size_t)ctx->D, (size_t)n,
                            hipMemcpyHostToDevice, ctx->stream));
    commit_labels(ctx, labels, n);
  });
}

LM_API lm_status lm_train_gather(lm_train_ctx* ctx, lm_ctx* det, const uint8_t* frames, int64_t pitch, int32_t n_frames,
                                 const lm_train_point* points, int32_t n_points) {
  return gather(ctx, det, frames, pitch, n_frames, points, n_points, false);
}

LM_API lm_status lm_train_gather_device(lm_train_ctx* ctx, lm_ctx* det, const uint8_t* d_frames, int64_t pitch,
                                        int32_t n_frames, const lm_train_point* points, int32_t n_points) {
  return gather(ctx, det, d_frames, pitch, n_frames, points, n_points, true);
}

LM_API lm_status lm_train_samples(lm_train_ctx* ctx, int32_t* n_pos, int32_t* n_neg) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (n_pos) *n_pos = (int32_t)ctx->n_pos;
  if (n_neg) *n_neg = (int32_t)(ctx->n - ctx->n_pos);
  return LM_OK;
}

LM_API lm_status lm_train_reset(lm_train_ctx* ctx) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  ctx->n = 0;
  ctx->n_pos = 0;
  ctx->h_y.clear();
  ctx->groups_set = false;
  return LM_OK;
}

LM_API lm_status lm_train_patches(lm_train_ctx* ctx, int32_t first, int32_t n, uint8_t* out_patches,
                                  int8_t* out_labels) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (first < 0 || n < 0 || (int64_t)first + n > ctx->n)
    return fail(LM_ERR_INVALID_ARGUMENT, "first .. first + n is outside the stored samples");
  return guarded([&] {
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    if (out_patches) {
      HIPCHK(hipMemcpy2DAsync(out_patches, (size_t)ctx->D, ctx->X.p + (size_t)first * (size_t)ctx->Dp, (size_t)ctx->Dp,
                              (size_t)ctx->D, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (out_labels) std::memcpy(out_labels, ctx->h_y.data() + first, (size_t)n);
  });
}

namespace {

// sample array oi = X~ (vector vi) with the matrix' bytes over div; with ai, sample array oai = sample array ai times it
void launch_xv(lm_train_ctx* c, const LmtProblems& M, int vi, double div, int ai, int oi, int oai, int gate) {
  const int L = lanes_per_sample(c->Dp);
  const int spb = kT / L * kXvS;
  const int pb = lmt_problem_block(c->D);
  const dim3 grid((unsigned)((c->n + spb - 1) / spb), (unsigned)((M.n + pb - 1) / pb));
  const size_t lds = sizeof(double) * (size_t)pb * (size_t)c->VL;
  hipLaunchKernelGGL(k_train_xv, grid, dim3(kT), lds, c->stream, c->X.p, c->n, c->Dp, L, M, pb, vi, div, ai, oi, oai,
                     gate);
}

// vector oi = vector bi + 2 X~^T (sample array ti), per problem
void launch_xt(lm_train_ctx* c, const LmtProblems& M, int ti, int bi, int oi, int gate) {
  const int nblk = (int)((c->n + LMT_XT_BLOCK - 1) / LMT_XT_BLOCK);
  const int nchunk = ((c->Dp >> 4) + 15) / 16;
  const int pb = lmt_problem_block(c->D);
  const dim3 grid(nchunk, nblk, (M.n + pb - 1) / pb);
  hipLaunchKernelGGL(k_train_xt, grid, dim3(kT), 0, c->stream, c->X.p, c->n, c->Dp, M, pb, ti, gate);
  hipLaunchKernelGGL(k_train_xt_reduce, dim3((c->VL + kT - 1) / kT, M.n), dim3(kT), 0, c->stream, M, nblk, c->Dp,
                     bi, oi, gate);
}

// The group bytes in device memory: zeros until groups are set.
void size_groups(lm_train_ctx* c) {
  if (c->group.p) return;
  c->group.alloc((size_t)c->max_samples);
  SET_SYNC(c->group.p, 0, (size_t)c->max_samples, c->stream);
}

// Why the problems cannot be solved, or "" (no device call).
std::string refuse_problems(const lm_train_ctx* c, const lm_train_problem* pr, int32_t n_problems) {
  if (n_problems < 1 || n_problems > LM_TRAIN_MAX_PROBLEMS)
    return "n_problems must be in 1.." + std::to_string(LM_TRAIN_MAX_PROBLEMS);
  std::vector<int64_t> in_group;
  for (int32_t q = 0; q < n_problems; ++q) {
    const std::string at = "problem " + std::to_string(q) + ": ";
    if (!(pr[q].c_pos > 0.0) || !std::isfinite(pr[q].c_pos) || !(pr[q].c_neg > 0.0) || !std::isfinite(pr[q].c_neg))
      return at + "c_pos and c_neg must be positive and finite";
    if (pr[q].reserved != 0) return at + "reserved must be 0";
    if (pr[q].held_out < -1 || pr[q].held_out >= LM_TRAIN_MAX_GROUPS)
      return at + "held_out must be in -1.." + std::to_string(LM_TRAIN_MAX_GROUPS - 1);
    if (pr[q].held_out < 0) continue;
    if (!c->groups_set) return at + "held_out without groups (lm_train_set_groups)";
    if (in_group.empty()) {
      in_group.assign(LM_TRAIN_MAX_GROUPS, 0);
      for (int64_t i = 0; i < c->n; ++i) in_group[c->h_group[(size_t)i]] += 1;
    }
    if (in_group[(size_t)pr[q].held_out] == c->n) return at + "its held-out group holds every stored sample";
  }
  return "";
}

// ---- a solve, step by step (solve_problems below)

// The arrays of a call of P problems on the stored samples: grown where they are too small, and bound.
LmtProblems bind_problems(lm_train_ctx* c, int P) {
  size_groups(c);
  const LmtLayout L = lmt_layout(c->n, c->VL);
  auto size = [P](auto& b, int64_t per_problem) {
    if (b.n < (size_t)P * (size_t)per_problem) b.alloc((size_t)P * (size_t)per_problem);
  };
  size(c->vec, L.vec);
  size(c->smp, L.smp);
  size(c->part, L.part);
  size(c->xtp, L.xtp);
  size(c->counts, L.counts);
  if (!c->prob.p) {
    c->prob.alloc(LM_TRAIN_MAX_PROBLEMS);
    c->ctl.alloc(LM_TRAIN_MAX_PROBLEMS);
    c->h_ctl.alloc(LM_TRAIN_MAX_PROBLEMS);
  }
  LmtProblems M;
  M.n = P;
  M.prob = c->prob.p;
  M.ctl = c->ctl.p;
  M.group = c->group.p;
  M.vec = c->vec.p;
  M.smp = c->smp.p;
  M.part = c->part.p;
  M.xtp = c->xtp.p;
  M.vec_stride = L.vec;
  M.smp_stride = L.smp;
  M.part_stride = L.part;
  M.xtp_stride = L.xtp;
  return M;
}

// The problems into device memory; each starts at w = 0 with a cleared control block.
void upload_problems(lm_train_ctx* c, const LmtProblems& M, const lm_train_problem* problems) {
  std::vector<LmtProb> pr((size_t)M.n);
  for (int q = 0; q < M.n; ++q) pr[(size_t)q] = LmtProb{problems[q].c_pos, problems[q].c_neg, problems[q].held_out, 0};
  COPY_SYNC(c->prob.p, pr.data(), sizeof(LmtProb) * pr.size(), hipMemcpyHostToDevice, c->stream);
  HIPCHK(hipMemsetAsync(M.vec, 0, sizeof(double) * (size_t)M.n * (size_t)M.vec_stride, c->stream));
  HIPCHK(hipMemsetAsync(M.ctl, 0, sizeof(LmtCtl) * (size_t)M.n, c->stream));
}

// One outer iteration of the problems that are not done: F, grad F and the
// active set at w; then, with `step`, the CG run and the line search.
void enqueue_outer(lm_train_ctx* c, const LmtProblems& M, double eps, bool first, bool step) {
  const int VL = c->VL, P = M.n;
  const int64_t N = c->n;
  const int nb = (int)lmt_layout(N, VL).nb;
  // CG steps enqueued per outer iteration: in exact arithmetic CG ends within
  // VL steps; past the cap the step taken is that of a shorter CG run
  const int cg_cap = c->D + 1 < 96 ? c->D + 1 : 96;
  launch_xv(c, M, V_W, 255.0, S_NONE, S_Z, S_NONE, GATE_CONVERGED);
  hipLaunchKernelGGL(k_train_coef, dim3(nb, P), dim3(kT), 0, c->stream, M, c->y.p, N, nb);
  launch_xt(c, M, S_T, V_W, V_G, GATE_CONVERGED);
  hipLaunchKernelGGL(k_train_eval, dim3(P), dim3(kT), 0, c->stream, M, VL, nb, eps, first ? 1 : 0);
  if (step) {
    for (int k = 0; k < cg_cap; ++k) {
      launch_xv(c, M, V_P, 255.0, S_A, S_U, S_AU, GATE_CG);
      launch_xt(c, M, S_AU, V_P, V_HP, GATE_CG);
      hipLaunchKernelGGL(k_train_cg_update, dim3(P), dim3(kT), 0, c->stream, M, VL);
    }
    launch_xv(c, M, V_D, 255.0, S_NONE, S_U, S_NONE, GATE_CONVERGED);
    hipLaunchKernelGGL(k_train_ls_partials, dim3(nb, P), dim3(kT), 0, c->stream, M, c->y.p, N, nb);
    hipLaunchKernelGGL(k_train_ls_pick, dim3(P), dim3(kT), 0, c->stream, M, VL, nb);
  }
  HIPCHK(hipGetLastError());
}

// The control blocks after outer iteration `it`, in c->h_ctl; a problem that
// is done now (converged, without a line-search step, or at max_iter) gets
// outer[q] = it.  True when every problem is done.
bool read_controls(lm_train_ctx* c, const LmtProblems& M, int it, int max_iter, std::vector<int>& outer) {
  COPY_SYNC(c->h_ctl.p, M.ctl, sizeof(LmtCtl) * (size_t)M.n, hipMemcpyDeviceToHost, c->stream);
  const LmtCtl* R = c->h_ctl.p;
  bool all = true;
  for (int q = 0; q < M.n; ++q) {
    if (outer[(size_t)q] < 0 && (R[q].converged || R[q].ls_fail || it >= max_iter)) outer[(size_t)q] = it;
    all = all && outer[(size_t)q] >= 0;
  }
  return all;
}

// The weights, the stats (from c->h_ctl) and, with `heldout`, the held-out
// counts of every problem.  A problem whose line search found no step is
// named in g_err, by its number when `numbered`; its w is unchanged since the
// evaluation, so the figures are its.
void read_results(lm_train_ctx* c, const LmtProblems& M, const std::vector<int>& outer, bool numbered, double* out_W,
                  double* out_rho, lm_train_stats* stats, lm_train_heldout* heldout) {
  const int VL = c->VL, P = M.n;
  const int nb = (int)lmt_layout(c->n, VL).nb;
  std::vector<int32_t> counts;
  if (heldout) {
    hipLaunchKernelGGL(k_train_heldout, dim3(nb, P), dim3(kT), 0, c->stream, M, c->y.p, c->n, nb, c->counts.p);
    HIPCHK(hipGetLastError());
    counts.resize((size_t)P * (size_t)nb * 4);
    COPY_SYNC(counts.data(), c->counts.p, sizeof(int32_t) * counts.size(), hipMemcpyDeviceToHost, c->stream);
  }
  std::vector<double> w((size_t)P * (size_t)VL);
  HIPCHK(hipMemcpy2DAsync(w.data(), sizeof(double) * (size_t)VL, M.vec, sizeof(double) * (size_t)M.vec_stride,
                          sizeof(double) * (size_t)VL, (size_t)P, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const LmtCtl* R = c->h_ctl.p;
  for (int q = 0; q < P; ++q) {
    const double* wq = w.data() + (size_t)q * (size_t)VL;
    for (int j = 0; j < c->D; ++j) out_W[(size_t)q * (size_t)c->D + (size_t)j] = wq[j] / 255.0;
    out_rho[q] = -wq[c->Dp];
    if (R[q].ls_fail && !R[q].converged)
      g_err = "the line search found no step" + (numbered ? " (problem " + std::to_string(q) + ")" : std::string());
    if (stats) {
      stats[q].objective = R[q].f;
      stats[q].grad_norm = R[q].gnorm;
      stats[q].grad_norm0 = R[q].gnorm0;
      stats[q].outer_iters = outer[(size_t)q];
      stats[q].cg_iters = R[q].cg_iters;
      stats[q].converged = R[q].converged;
      stats[q].n_active = R[q].n_active;
    }
    if (heldout) {
      int32_t s[4] = {0, 0, 0, 0};
      for (int b = 0; b < nb; ++b)  // in block order
        for (int k = 0; k < 4; ++k) s[k] += counts[((size_t)q * (size_t)nb + (size_t)b) * 4 + (size_t)k];
      heldout[q] = lm_train_heldout{s[0], s[1], s[2], s[3]};
    }
  }
}

// The solver: P checked problems on the stored samples.  The host reads the
// control blocks once per outer iteration and stops when every problem is done.
void solve_problems(lm_train_ctx* c, const lm_train_problem* problems, int P, double eps, int max_iter, bool numbered,
                    double* out_W, double* out_rho, lm_train_stats* stats, lm_train_heldout* heldout) {
  HIPCHK(hipSetDevice(c->device));
  const LmtProblems M = bind_problems(c, P);
  upload_problems(c, M, problems);
  std::vector<int> outer((size_t)P, -1);  // a problem's outer iterations, once it is done
  for (int it = 0;; ++it) {
    enqueue_outer(c, M, eps, it == 0, it < max_iter);
    if (read_controls(c, M, it, max_iter, outer)) break;
  }
  read_results(c, M, outer, numbered, out_W, out_rho, stats, heldout);
}

}  // namespace

LM_API lm_status lm_train_set_groups(lm_train_ctx* ctx, const int32_t* groups, int32_t n) {
  if (!ctx || !groups) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  if (n != ctx->n)
    return fail(LM_ERR_INVALID_ARGUMENT,
                "n is " + std::to_string(n) + ", the context holds " + std::to_string(ctx->n) + " samples");
  for (int32_t i = 0; i < n; ++i)
    if (groups[i] < 0 || groups[i] >= LM_TRAIN_MAX_GROUPS)
      return fail(LM_ERR_INVALID_ARGUMENT, "group " + std::to_string(i) + " is " + std::to_string(groups[i]) +
                                               ": must be in 0.." + std::to_string(LM_TRAIN_MAX_GROUPS - 1));
  return guarded([&] {
    std::vector<uint8_t> g((size_t)n);
    for (int32_t i = 0; i < n; ++i) g[(size_t)i] = (uint8_t)groups[i];
    HIPCHK(hipSetDevice(ctx->device));
    size_groups(ctx);
    COPY_SYNC(ctx->group.p, g.data(), (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    ctx->h_group.swap(g);
    ctx->groups_set = true;
  });
}

LM_API int32_t lm_train_problem_block(lm_train_ctx* ctx) { return ctx ? lmt_problem_block(ctx->D) : 0; }

LM_API lm_status lm_train_solve_many(lm_train_ctx* ctx, const lm_train_problem* problems, int32_t n_problems,
                                     double eps, int32_t max_iter, double* out_W, double* out_rho,
                                     lm_train_stats* stats, lm_train_heldout* heldout) {
  if (!ctx || !problems || !out_W || !out_rho) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(LM_ERR_INVALID_ARGUMENT, "eps must be positive and finite");
  if (max_iter < 0) return fail(LM_ERR_INVALID_ARGUMENT, "max_iter is negative");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  const std::string why = refuse_problems(ctx, problems, n_problems);
  if (!why.empty()) return fail(LM_ERR_INVALID_ARGUMENT, why);
  return guarded([&] { solve_problems(ctx, problems, n_problems, eps, max_iter, true, out_W, out_rho, stats, heldout); });
}

// The one-problem call {c_pos, c_neg, no held-out group}, with its own refusals.
LM_API lm_status lm_train_solve(lm_train_ctx* ctx, double c_pos, double c_neg, double eps, int32_t max_iter,
                                double* out_W, double* out_rho, lm_train_stats* stats) {
  if (!ctx || !out_W || !out_rho) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (!(c_pos > 0.0) || !std::isfinite(c_pos) || !(c_neg > 0.0) || !std::isfinite(c_neg))
    return fail(LM_ERR_INVALID_ARGUMENT, "c_pos and c_neg must be positive and finite");
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(LM_ERR_INVALID_ARGUMENT, "eps must be positive and finite");
  if (max_iter < 0) return fail(LM_ERR_INVALID_ARGUMENT, "max_iter is negative");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  return guarded([&] {
    const lm_train_problem one{c_pos, c_neg, -1, 0};
    solve_problems(ctx, &one, 1, eps, max_iter, false, out_W, out_rho, stats, nullptr);
  });
}

// One X~ v pass as a one-problem call: the model in problem 0's hp (scratch outside a solve), the margins in its z.
LM_API lm_status lm_train_margins(lm_train_ctx* ctx, const double* W, double rho, double* out_z) {
  if (!ctx || !W || !out_z) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  return guarded([&] {
    lm_train_ctx* c = ctx;
    HIPCHK(hipSetDevice(c->device));
    const LmtProblems M = bind_problems(c, 1);
    std::vector<double> v((size_t)c->VL, 0.0);
    for (int j = 0; j < c->D; ++j) v[(size_t)j] = W[j];
    v[(size_t)c->Dp] = -rho;
    COPY_SYNC(M.vec + (size_t)V_HP * (size_t)c->VL, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, c->stream);
    launch_xv(c, M, V_HP, 1.0, S_NONE, S_Z, S_NONE, GATE_NONE);
    HIPCHK(hipGetLastError());
    COPY_SYNC(out_z, M.smp + (size_t)S_Z * (size_t)c->n, sizeof(double) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
  });
}

LM_API void* lm_train_stream(lm_train_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
