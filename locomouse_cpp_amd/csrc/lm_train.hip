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
//   k_train_xv         out = X~ v: L = 2^k lanes per sample (L >= D / 16, at
//                      most 64) and four consecutive samples per lane group,
//                      so 256 / L samples per wave; v in LDS; a lane loads 16
//                      bytes of each of its samples' rows at a time; the L
//                      lanes' sums are folded by xor butterflies (the same
//                      pairs whatever the lane, so every lane has the sum).
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
//
// An outer iteration is enqueued whole: the CG steps (a fixed number of
// them, each a no-op once the residual is small) and the line search read
// their flags from the control block in device memory, and the host reads
// that block once per outer iteration.  Every sum is taken in an order that
// depends on N and D alone: strided per-thread sums, then a binary tree in
// LDS; blocks of samples in index order.  No atomics.
//
// Safety: sample rows are read at i * Dp for i < N <= max_samples, which
// sizes the matrix; vectors have VL entries and are indexed below VL; the
// per-block partials are sized from N before a launch.  The gather writes
// rows n0 .. n0 + n_points - 1 with n0 + n_points <= max_samples, and its
// points' frame indices and coordinates are checked on the host; taps outside
// the corrected image read nothing.
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

DEV bool gated(const LmtCtl* ctl, int gate) {
  return (gate == GATE_CG && ctl->cg_done) || (gate == GATE_CONVERGED && (ctl->converged || ctl->ls_fail));
}

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

__global__ __launch_bounds__(kT) void k_train_xv(const uint8_t* __restrict__ X, int64_t N, int Dp, int L,
                                                 const double* __restrict__ v, double div,
                                                 const double* __restrict__ a, double* __restrict__ out,
                                                 double* __restrict__ out_a, const LmtCtl* ctl, int gate) {
  if (gated(ctl, gate)) return;
  extern __shared__ double sv[];  // VL doubles
  for (int j = threadIdx.x; j <= Dp; j += kT) sv[j] = v[j];
  __syncthreads();
  const int gl = threadIdx.x & (L - 1);
  // the group's kXvS consecutive samples: their loads are in flight together, and an entry of v is read once for all
  const int64_t i0 = ((int64_t)blockIdx.x * (kT / L) + threadIdx.x / L) * kXvS;
  const int ncg = Dp >> 4;
  double acc[kXvS];
#pragma unroll
  for (int s = 0; s < kXvS; ++s) acc[s] = 0.0;
  for (int g = gl; g < ncg; g += L) {
    uint4 q[kXvS];
#pragma unroll
    for (int s = 0; s < kXvS; ++s)
      q[s] = i0 + s < N ? reinterpret_cast<const uint4*>(X + (i0 + s) * Dp)[g] : make_uint4(0, 0, 0, 0);
    const double* w = sv + 16 * g;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double wk = w[k];
#pragma unroll
      for (int s = 0; s < kXvS; ++s) {
        const uint32_t word = (k >> 2) == 0 ? q[s].x : (k >> 2) == 1 ? q[s].y : (k >> 2) == 2 ? q[s].z : q[s].w;
        acc[s] += (double)((word >> (8 * (k & 3))) & 255u) * wk;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kXvS; ++s) {
    double r = acc[s];
    for (int o = L >> 1; o > 0; o >>= 1) r += __shfl_xor(r, o);
    if (gl == 0 && i0 + s < N) {
      const double z = r / div + sv[Dp];
      out[i0 + s] = z;
      if (a) out_a[i0 + s] = a[i0 + s] * z;
    }
  }
}

__global__ __launch_bounds__(kT) void k_train_xt(const uint8_t* __restrict__ X, int64_t N, int Dp,
                                                 const double* __restrict__ t, double* __restrict__ partial,
                                                 const LmtCtl* ctl, int gate) {
  if (gated(ctl, gate)) return;
  __shared__ double red[16][kXtCols];
  __shared__ double redb[16];
  const int cgx = threadIdx.x & 15, sy = threadIdx.x >> 4;
  const int g = blockIdx.x * 16 + cgx;  // column group of 16
  const bool cols = g < (Dp >> 4);
  const bool bias = blockIdx.x == 0 && cgx == 0;
  const int64_t i0 = (int64_t)blockIdx.y * LMT_XT_BLOCK;
  const int64_t i1 = i0 + LMT_XT_BLOCK < N ? i0 + LMT_XT_BLOCK : N;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  double tb = 0.0;
  if (cols || bias) {
#pragma unroll 4
    for (int64_t i = i0 + sy; i < i1; i += 16) {
      const double ti = t[i];
      if (bias) tb += ti;
      if (cols) {
        const uint4 q = *reinterpret_cast<const uint4*>(X + i * Dp + 16 * g);
        const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] += ti * (double)((word[k >> 2] >> (8 * (k & 3))) & 255u);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) red[sy][cgx * 16 + k] = acc[k];
  if (bias) redb[sy] = tb;
  __syncthreads();
  const int VL = Dp + 1;
  double* prow = partial + (int64_t)blockIdx.y * VL;
  const int c = blockIdx.x * kXtCols + threadIdx.x;
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

__global__ __launch_bounds__(kT) void k_train_xt_reduce(const double* __restrict__ partial, int nblk, int Dp,
                                                        const double* __restrict__ base, double* __restrict__ out,
                                                        const LmtCtl* ctl, int gate) {
  if (gated(ctl, gate)) return;
  const int VL = Dp + 1;
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= VL) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * VL + j];
  if (j < Dp) s = s / 255.0;
  out[j] = base[j] + 2.0 * s;
}

__global__ __launch_bounds__(kT) void k_train_coef(const double* __restrict__ z, const int8_t* __restrict__ y, int64_t N,
                                                   double c_pos, double c_neg, double* __restrict__ a,
                                                   double* __restrict__ t, double* __restrict__ part_loss,
                                                   double* __restrict__ part_act) {
  __shared__ double sh[kT];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  double loss = 0.0, act = 0.0;
  if (i < N) {
    double ti;
    const double ai = lmt_coef(y[i], z[i], c_pos, c_neg, &ti, &loss);
    a[i] = ai;
    t[i] = ti;
    act = ai != 0.0 ? 1.0 : 0.0;
  }
  const double sl = block_sum(loss, sh);
  const double sa = block_sum(act, sh);  // (counts below 2^53 are exact in a double)
  if (threadIdx.x == 0) {
    part_loss[blockIdx.x] = sl;
    part_act[blockIdx.x] = sa;
  }
}

// F and |grad F| at w from the parts; sets the flags; d = 0, r = p = -g.
__global__ __launch_bounds__(kT) void k_train_eval(const double* __restrict__ w, const double* __restrict__ g, int VL,
                                                   const double* __restrict__ part_loss,
                                                   const double* __restrict__ part_act, int nb, double eps, int first,
                                                   double* __restrict__ d, double* __restrict__ r,
                                                   double* __restrict__ p, LmtCtl* ctl) {
  __shared__ double sh[kT];
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
  const double loss = block_sum_array(part_loss, nb, sh);
  const double act = block_sum_array(part_act, nb, sh);
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
__global__ __launch_bounds__(kT) void k_train_cg_update(double* __restrict__ d, double* __restrict__ r,
                                                        double* __restrict__ p, const double* __restrict__ hp, int VL,
                                                        LmtCtl* ctl) {
  if (ctl->cg_done) return;
  __shared__ double sh[kT];
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
__global__ __launch_bounds__(kT) void k_train_ls_partials(const double* __restrict__ z, const double* __restrict__ xd,
                                                          const int8_t* __restrict__ y, int64_t N, double c_pos,
                                                          double c_neg, double* __restrict__ lspart,
                                                          const LmtCtl* ctl) {
  if (gated(ctl, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = i < N;
  const int yi = valid ? y[i] : 1;
  const double zi = valid ? z[i] : 0.0, xi = valid ? xd[i] : 0.0;
  double lambda = 1.0;
  for (int k = 0; k < LMT_LS_STEPS; ++k, lambda *= 0.5) {
    const double v = valid ? lmt_ls_delta(yi, zi, xi, lambda, c_pos, c_neg) : 0.0;
    const double s = block_sum(v, sh);
    if (threadIdx.x == 0) lspart[(int64_t)blockIdx.x * LMT_LS_STEPS + k] = s;
  }
}

// The first lambda that satisfies Armijo; w += lambda d.
__global__ __launch_bounds__(kT) void k_train_ls_pick(double* __restrict__ w, const double* __restrict__ g,
                                                      const double* __restrict__ d, int VL,
                                                      const double* __restrict__ lspart, int nb, LmtCtl* ctl) {
  if (gated(ctl, GATE_CONVERGED)) return;
  __shared__ double sh[kT];
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
  // solver (sized at the first solve for the samples then stored)
  DevBuf<double> vec;   // w, g, d, r, p, hp: 6 x VL
  DevBuf<double> smp;   // z, u, a, t, au: 5 x cap_n
  DevBuf<double> part;  // part_loss, part_act (nb each), lspart (nb x LMT_LS_STEPS)
  DevBuf<double> xtp;   // k_train_xt's partials, nblk x VL
  int64_t cap_n = 0;
  DevBuf<LmtCtl> ctl;
  HostBuf<LmtCtl> h_ctl;
  HostBuf<double> h_vec;  // VL
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

void launch_xv(lm_train_ctx* c, const double* v, double div, const double* a, double* out, double* out_a, int gate) {
  const int L = lanes_per_sample(c->Dp);
  const int spb = kT / L * kXvS;
  const unsigned grid = (unsigned)((c->n + spb - 1) / spb);
  hipLaunchKernelGGL(k_train_xv, dim3(grid), dim3(kT), sizeof(double) * (size_t)c->VL, c->stream, c->X.p, c->n, c->Dp, L,
                     v, div, a, out, out_a, c->ctl.p, gate);
}

// out = base + 2 X~^T t
void launch_xt(lm_train_ctx* c, const double* t, const double* base, double* out, int gate) {
  const int nblk = (int)((c->n + LMT_XT_BLOCK - 1) / LMT_XT_BLOCK);
  const int nchunk = ((c->Dp >> 4) + 15) / 16;
  hipLaunchKernelGGL(k_train_xt, dim3(nchunk, nblk), dim3(kT), 0, c->stream, c->X.p, c->n, c->Dp, t, c->xtp.p, c->ctl.p,
                     gate);
  hipLaunchKernelGGL(k_train_xt_reduce, dim3((c->VL + kT - 1) / kT), dim3(kT), 0, c->stream, c->xtp.p, nblk, c->Dp, base,
                     out, c->ctl.p, gate);
}

void size_solver(lm_train_ctx* c) {
  if (!c->vec.p) {
    c->vec.alloc(6 * (size_t)c->VL);
    c->ctl.alloc(1);
    c->h_ctl.alloc(1);
    c->h_vec.alloc((size_t)c->VL);
  }
  if (c->cap_n < c->n) {
    const size_t nb = (size_t)((c->n + kT - 1) / kT);
    const size_t nblk = (size_t)((c->n + LMT_XT_BLOCK - 1) / LMT_XT_BLOCK);
    c->smp.alloc(5 * (size_t)c->n);
    c->part.alloc(nb * (2 + LMT_LS_STEPS));
    c->xtp.alloc(nblk * (size_t)c->VL);
    c->cap_n = c->n;
  }
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

LM_API lm_status lm_train_solve(lm_train_ctx* ctx, double c_pos, double c_neg, double eps, int32_t max_iter,
                                double* out_W, double* out_rho, lm_train_stats* stats) {
  if (!ctx || !out_W || !out_rho) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (!(c_pos > 0.0) || !std::isfinite(c_pos) || !(c_neg > 0.0) || !std::isfinite(c_neg))
    return fail(LM_ERR_INVALID_ARGUMENT, "c_pos and c_neg must be positive and finite");
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(LM_ERR_INVALID_ARGUMENT, "eps must be positive and finite");
  if (max_iter < 0) return fail(LM_ERR_INVALID_ARGUMENT, "max_iter is negative");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  return guarded([&] {
    lm_train_ctx* c = ctx;
    HIPCHK(hipSetDevice(c->device));
    size_solver(c);
    const int VL = c->VL;
    const int64_t N = c->n;
    double *w = c->vec.p, *g = w + VL, *d = g + VL, *r = d + VL, *p = r + VL, *hp = p + VL;
    double *z = c->smp.p, *u = z + N, *a = u + N, *t = a + N, *au = t + N;
    const int nb = (int)((N + kT - 1) / kT);
    double *part_loss = c->part.p, *part_act = part_loss + nb, *lspart = part_act + nb;
    // CG steps enqueued per outer iteration: in exact arithmetic CG ends within
    // VL steps; past the cap the step taken is that of a shorter CG run
    const int cg_cap = c->D + 1 < 96 ? c->D + 1 : 96;
    HIPCHK(hipMemsetAsync(w, 0, sizeof(double) * 6 * (size_t)VL, c->stream));
    HIPCHK(hipMemsetAsync(c->ctl.p, 0, sizeof(LmtCtl), c->stream));
    int it = 0;
    for (;; ++it) {
      // F, grad F and the active set at w
      launch_xv(c, w, 255.0, nullptr, z, nullptr, GATE_NONE);
      hipLaunchKernelGGL(k_train_coef, dim3(nb), dim3(kT), 0, c->stream, z, c->y.p, N, c_pos, c_neg, a, t, part_loss,
                         part_act);
      launch_xt(c, t, w, g, GATE_NONE);
      hipLaunchKernelGGL(k_train_eval, dim3(1), dim3(kT), 0, c->stream, w, g, VL, part_loss, part_act, nb, eps,
                         it == 0 ? 1 : 0, d, r, p, c->ctl.p);
      if (it < max_iter) {
        for (int k = 0; k < cg_cap; ++k) {
          launch_xv(c, p, 255.0, a, u, au, GATE_CG);
          launch_xt(c, au, p, hp, GATE_CG);
          hipLaunchKernelGGL(k_train_cg_update, dim3(1), dim3(kT), 0, c->stream, d, r, p, hp, VL, c->ctl.p);
        }
        launch_xv(c, d, 255.0, nullptr, u, nullptr, GATE_CONVERGED);
        hipLaunchKernelGGL(k_train_ls_partials, dim3(nb), dim3(kT), 0, c->stream, z, u, c->y.p, N, c_pos, c_neg, lspart,
                           c->ctl.p);
        hipLaunchKernelGGL(k_train_ls_pick, dim3(1), dim3(kT), 0, c->stream, w, g, d, VL, lspart, nb, c->ctl.p);
      }
      HIPCHK(hipGetLastError());
      COPY_SYNC(c->h_ctl.p, c->ctl.p, sizeof(LmtCtl), hipMemcpyDeviceToHost, c->stream);
      if (c->h_ctl.p->converged || c->h_ctl.p->ls_fail || it >= max_iter) break;
    }
    const LmtCtl& R = *c->h_ctl.p;
    if (R.ls_fail && !R.converged) {  // w is unchanged since the evaluation: the figures are its
      g_err = "the line search found no step";
    }
    COPY_SYNC(c->h_vec.p, w, sizeof(double) * (size_t)VL, hipMemcpyDeviceToHost, c->stream);
    for (int j = 0; j < c->D; ++j) out_W[j] = c->h_vec.p[j] / 255.0;
    *out_rho = -c->h_vec.p[c->Dp];
    if (stats) {
      stats->objective = R.f;
      stats->grad_norm = R.gnorm;
      stats->grad_norm0 = R.gnorm0;
      stats->outer_iters = it;
      stats->cg_iters = R.cg_iters;
      stats->converged = R.converged;
      stats->n_active = R.n_active;
    }
  });
}

LM_API lm_status lm_train_margins(lm_train_ctx* ctx, const double* W, double rho, double* out_z) {
  if (!ctx || !W || !out_z) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (ctx->n < 1) return fail(LM_ERR_INVALID_ARGUMENT, "the context holds no samples");
  return guarded([&] {
    lm_train_ctx* c = ctx;
    HIPCHK(hipSetDevice(c->device));
    size_solver(c);
    for (int j = 0; j < c->VL; ++j) c->h_vec.p[j] = j < c->D ? W[j] : 0.0;
    c->h_vec.p[c->Dp] = -rho;
    double* hp = c->vec.p + 5 * (size_t)c->VL;  // (scratch outside a solve)
    COPY_SYNC(hp, c->h_vec.p, sizeof(double) * (size_t)c->VL, hipMemcpyHostToDevice, c->stream);
    launch_xv(c, hp, 1.0, nullptr, c->smp.p, nullptr, GATE_NONE);
    HIPCHK(hipGetLastError());
    COPY_SYNC(out_z, c->smp.p, sizeof(double) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream);
  });
}

LM_API void* lm_train_stream(lm_train_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
