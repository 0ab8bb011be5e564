// lm_calib.hip — the marker records of the calibration estimate
// (include/locomouse_calib.h; the definition is csrc/lm_calib_core.h).
//
//   k_calib_record   one workgroup of 256 threads per (frame, view).  A view
//                    is whole rows, so its pixels are one contiguous range of
//                    the frame and of the background: the sweep is flat.  Each
//                    thread keeps the largest d = max(0, frame - background)
//                    it met with the first index that held it (its indices
//                    ascend, so "strictly greater replaces" keeps the first)
//                    and counts d > threshold; the middle of the range goes in
//                    16-byte loads when the frame's base is 16-byte aligned
//                    (the background's always is), the ends and unaligned
//                    frames in bytes.  The 64-bit key (d << 32) | ~index is
//                    max-reduced over the wave by shuffles and over the four
//                    waves through LDS behind the one barrier, which also
//                    settles the first-position tie; then wave 0 sums the
//                    window's moments in 64-bit integers and lane 0 writes the
//                    record.
//
// Safety: frame f < n is read at f * pitch + i for i < rows * cols <= pitch
// only (checked on the host before anything is launched), the background at
// i < rows * cols, its size; 16-byte loads stay inside [a0, a1), a subrange of
// the view; the record index 2 * (first + f) + view is below the capacity the
// host grew the buffer to before the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

#include "locomouse_calib.h"
#include "lm_calib_core.h"
#include "lm_host.h"

static_assert(sizeof(lm_calib_record) == 48, "the record's layout is part of the ABI");

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct LmcBest {  // a thread's largest d so far and the first index that held it
  int d;
  uint32_t i;
};

__device__ __forceinline__ void lmc_take(LmcBest& b, int& cnt, uint32_t f, uint32_t g, uint32_t i, int thr) {
  const int d = lmc_diff(f, g);
  cnt += d > thr;
  if (d > b.d) {
    b.d = d;
    b.i = i;
  }
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, off);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_xor((unsigned long long)v, off);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_calib_record(const uint8_t* __restrict__ frames, int64_t pitch,
                                                           const uint8_t* __restrict__ bkg, int rows, int cols,
                                                           int split_row, int thr, int radius,
                                                           lm_calib_record* __restrict__ out) {
  __shared__ uint64_t s_key[kWaves];
  __shared__ int s_cnt[kWaves];
  const int f = blockIdx.x >> 1, view = blockIdx.x & 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* __restrict__ F = frames + (int64_t)f * pitch;
  int vr0, vr1;
  lmc_view_rows(view, rows, split_row, &vr0, &vr1);
  const uint32_t i0 = (uint32_t)vr0 * (uint32_t)cols, i1 = (uint32_t)vr1 * (uint32_t)cols;
  // [a0, a1): the part swept in 16-byte loads
  uint32_t a0 = i0, a1 = i0;
  if ((((uintptr_t)F | (uintptr_t)bkg) & 15) == 0) {
    a0 = (i0 + 15u) & ~15u;
    a1 = i1 & ~15u;
    if (a1 < a0) a0 = a1 = i0;
  }
  LmcBest best{-1, 0};
  int cnt = 0;
  for (uint32_t i = i0 + tid; i < a0; i += kThreads) lmc_take(best, cnt, F[i], bkg[i], i, thr);
#pragma unroll 2
  for (uint32_t i = a0 + 16u * tid; i < a1; i += 16u * kThreads) {
    const uint4 fv = *reinterpret_cast<const uint4*>(F + i);
    const uint4 gv = *reinterpret_cast<const uint4*>(bkg + i);
    const uint32_t fw[4] = {fv.x, fv.y, fv.z, fv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lmc_take(best, cnt, (fw[w] >> (8 * k)) & 255u, (gw[w] >> (8 * k)) & 255u, i + 4 * w + k, thr);
  }
  for (uint32_t i = a1 + tid; i < i1; i += kThreads) lmc_take(best, cnt, F[i], bkg[i], i, thr);

  uint64_t key = best.d >= 0 ? lmc_key((uint32_t)best.d, best.i) : 0;  // (a real key is above 0: index < 2^31)
  key = wave_max(key);
  cnt = (int)wave_sum((uint64_t)(uint32_t)cnt);
  if (lane == 0) {
    s_key[wave] = key;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (wave != 0) return;
  key = s_key[0];
  cnt = s_cnt[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {
    key = s_key[k] > key ? s_key[k] : key;
    cnt += s_cnt[k];
  }
  const uint32_t idx = lmc_key_index(key);
  const int px = (int)(idx % (uint32_t)cols), py = (int)(idx / (uint32_t)cols);
  const LmcWindow w = lmc_window(px, py, radius, vr0, vr1, cols);
  const uint32_t ww = (uint32_t)(w.c1 - w.c0 + 1), wn = ww * (uint32_t)(w.r1 - w.r0 + 1);
  uint64_t n_in = 0, S = 0, Sx = 0, Sy = 0;
#pragma unroll 4
  for (uint32_t j = lane; j < wn; j += 64) {
    const uint32_t r = (uint32_t)w.r0 + j / ww, c = (uint32_t)w.c0 + j % ww;
    const size_t i = (size_t)r * (uint32_t)cols + c;
    const int d = lmc_diff(F[i], bkg[i]);
    if (d > thr) {
      n_in += 1;
      S += (uint32_t)d;
      Sx += (uint64_t)((uint32_t)d * c);  // 255 * 65535 fits 32 bits
      Sy += (uint64_t)((uint32_t)d * r);
    }
  }
  n_in = wave_sum(n_in);
  S = wave_sum(S);
  Sx = wave_sum(Sx);
  Sy = wave_sum(Sy);
  if (lane == 0) {
    lm_calib_record rec;
    rec.peak = (int32_t)lmc_key_peak(key);
    rec.px = px;
    rec.py = py;
    rec.n_above = cnt;
    rec.n_in = (int32_t)n_in;
    rec.clipped = w.clipped;
    rec.S = (int64_t)S;
    rec.Sx = (int64_t)Sx;
    rec.Sy = (int64_t)Sy;
    out[2 * f + view] = rec;
  }
}

lm_calib_opts default_opts() {
  lm_calib_opts o;
  o.threshold = 40;
  o.radius = 12;
  o.min_peak = 80;
  o.min_area = 12;
  o.max_stray = 8;
  o.reserved = 0;
  return o;
}

}  // namespace

struct lm_calib_ctx {
  int device = 0;
  int rows = 0, cols = 0, split_row = 0, max_batch = 0;
  lm_calib_opts opts{};
  uint32_t npix = 0;
  int64_t frames = 0, capacity = 0;  // records kept / room for, in frames
  hipStream_t stream = nullptr;
  DevBuf<uint8_t> d_bkg;
  DevBuf<uint8_t> d_stage;  // lm_calib_push: the batch's frames, tightly packed (allocated at the first host push)
  DevBuf<lm_calib_record> d_rec;
  ~lm_calib_ctx() {
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

void check_push(const lm_calib_ctx* c, int64_t pitch, int n) {
  if (n < 0 || n > c->max_batch) throw std::invalid_argument("n exceeds the context's max_batch");
  if (pitch < (int64_t)c->npix) throw std::invalid_argument("pitch is smaller than a frame");
  if (c->frames + n > LM_CALIB_MAX_FRAMES)
    throw std::invalid_argument("the push would take the frame count past LM_CALIB_MAX_FRAMES (" +
                                std::to_string(LM_CALIB_MAX_FRAMES) + "): " + std::to_string(c->frames) + " + " +
                                std::to_string(n));
}

// Room for `need` frames' records, the kept ones carried over.
void reserve(lm_calib_ctx* c, int64_t need) {
  if (need <= c->capacity) return;
  const int64_t cap = std::min<int64_t>(std::max<int64_t>(need, 2 * c->capacity), LM_CALIB_MAX_FRAMES);
  DevBuf<lm_calib_record> grown;
  grown.alloc((size_t)cap * 2);
  if (c->frames > 0)
    COPY_SYNC(grown.p, c->d_rec.p, sizeof(lm_calib_record) * 2 * (size_t)c->frames, hipMemcpyDeviceToDevice, c->stream);
  else
    HIPCHK(hipStreamSynchronize(c->stream));
  std::swap(grown.p, c->d_rec.p);
  std::swap(grown.n, c->d_rec.n);
  c->capacity = cap;
}

void launch_record(lm_calib_ctx* c, const uint8_t* d_frames, int64_t pitch, int n) {
  reserve(c, c->frames + n);
  hipLaunchKernelGGL(k_calib_record, dim3(2u * (unsigned)n), dim3(kThreads), 0, c->stream, d_frames, pitch, c->d_bkg.p,
                     c->rows, c->cols, c->split_row, c->opts.threshold, c->opts.radius, c->d_rec.p + 2 * c->frames);
  HIPCHK(hipGetLastError());
  c->frames += n;
}

}  // namespace

LM_API void lm_calib_default_opts(lm_calib_opts* out) {
  if (out) *out = default_opts();
}

LM_API lm_status lm_calib_create(int32_t device, int32_t rows, int32_t cols, int32_t split_row, int32_t max_batch,
                                 const lm_calib_opts* opts, lm_calib_ctx** out) {
  if (!out) return fail(LM_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (max_batch <= 0 || max_batch > 65535) return fail(LM_ERR_INVALID_ARGUMENT, "max_batch must be in 1..65535");
  if (const char* why = lmc_check_shape(rows, cols, split_row)) return fail(LM_ERR_INVALID_ARGUMENT, why);
  const lm_calib_opts o = opts ? *opts : default_opts();
  if (const char* why = lmc_check_opts(o)) return fail(LM_ERR_INVALID_ARGUMENT, why);
  lm_calib_ctx* c = new lm_calib_ctx();
  lm_status s = guarded([&] {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw HipError("invalid HIP device index");
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->rows = rows;
    c->cols = cols;
    c->split_row = split_row;
    c->max_batch = max_batch;
    c->opts = o;
    c->npix = (uint32_t)rows * (uint32_t)cols;
    c->d_bkg.alloc(c->npix);
    SET_SYNC(c->d_bkg.p, 0, c->npix, c->stream);
    reserve(c, std::max(max_batch, 1024));
  });
  if (s != LM_OK) {
    delete c;
    return s;
  }
  *out = c;
  return LM_OK;
}

LM_API void lm_calib_destroy(lm_calib_ctx* ctx) { delete ctx; }

LM_API lm_status lm_calib_set_background(lm_calib_ctx* ctx, const uint8_t* h_bkg) {
  if (!ctx || !h_bkg) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    // (the stream runs the earlier pushes' kernels before this copy overwrites what they read)
    COPY_SYNC(ctx->d_bkg.p, h_bkg, ctx->npix, hipMemcpyHostToDevice, ctx->stream);
  });
}

LM_API lm_status lm_calib_push(lm_calib_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n) {
  if (!ctx || !h_frames) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_push(ctx, pitch, n);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t fb = ctx->npix;
    if (!ctx->d_stage.p) ctx->d_stage.alloc(fb * (size_t)ctx->max_batch);
    // (the stream runs the previous push's kernel before this copy overwrites what it reads)
    HIPCHK(hipMemcpy2DAsync(ctx->d_stage.p, fb, h_frames, (size_t)pitch, fb, (size_t)n, hipMemcpyHostToDevice,
                            ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the caller's frames are free again
    launch_record(ctx, ctx->d_stage.p, (int64_t)fb, n);
  });
}

LM_API lm_status lm_calib_push_device(lm_calib_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n) {
  if (!ctx || !d_frames) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_push(ctx, pitch, n);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    launch_record(ctx, d_frames, pitch, n);
  });
}

LM_API int64_t lm_calib_frames(lm_calib_ctx* ctx) { return ctx ? ctx->frames : -1; }

LM_API lm_status lm_calib_read(lm_calib_ctx* ctx, int64_t first, int32_t n, lm_calib_record* out) {
  if (!ctx || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (first < 0 || n < 0 || first + n > ctx->frames)
    return fail(LM_ERR_INVALID_ARGUMENT, "frames " + std::to_string(first) + " .. " + std::to_string(first + n) +
                                             " were not all pushed (" + std::to_string(ctx->frames) + " so far)");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    if (n == 0) {
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return;
    }
    COPY_SYNC(out, ctx->d_rec.p + 2 * first, sizeof(lm_calib_record) * 2 * (size_t)n, hipMemcpyDeviceToHost,
              ctx->stream);
  });
}

LM_API lm_status lm_calib_reset(lm_calib_ctx* ctx) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->frames = 0;
  });
}

LM_API void* lm_calib_stream(lm_calib_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// ---- the fit and the map: no device

LM_API lm_status lm_calib_fit(const lm_calib_record* records, int32_t n_frames, int32_t rows, int32_t cols,
                              int32_t split_row, const lm_calib_opts* opts, int32_t degree, double max_resid,
                              lm_calib_fit_result* result) {
  if (!records || !result) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (n_frames < 0) return fail(LM_ERR_INVALID_ARGUMENT, "n_frames must not be negative");
  if (const char* why = lmc_check_shape(rows, cols, split_row)) return fail(LM_ERR_INVALID_ARGUMENT, why);
  const lm_calib_opts o = opts ? *opts : default_opts();
  if (const char* why = lmc_check_opts(o)) return fail(LM_ERR_INVALID_ARGUMENT, why);
  if (degree < 1 || degree > LM_CALIB_MAX_DEGREE) return fail(LM_ERR_INVALID_ARGUMENT, "degree must be 1, 2 or 3");
  if (!(max_resid > 0.0)) return fail(LM_ERR_INVALID_ARGUMENT, "max_resid must be positive");
  return guarded([&] {
    const std::string why = lmc_fit(records, n_frames, cols, o, degree, max_resid, result);
    if (!why.empty()) throw std::runtime_error(why);
  });
}

LM_API lm_status lm_calib_map(const lm_calib_fit_result* result, int32_t rows, int32_t cols, int32_t split_row,
                              int32_t* map_out, int32_t* view_boxes_out) {
  if (!result || !map_out || !view_boxes_out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = lmc_check_shape(rows, cols, split_row)) return fail(LM_ERR_INVALID_ARGUMENT, why);
  if (result->degree < 1 || result->degree > LM_CALIB_MAX_DEGREE)
    return fail(LM_ERR_INVALID_ARGUMENT, "the fit's degree must be 1, 2 or 3");
  if (!(result->lo <= result->hi)) return fail(LM_ERR_INVALID_ARGUMENT, "the fit's range is empty");
  return guarded([&] {
    const std::string why = lmc_map(*result, rows, cols, split_row, map_out, view_boxes_out);
    if (!why.empty()) throw std::runtime_error(why);
  });
}
