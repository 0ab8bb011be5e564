// lm_bkg.hip — the background estimate (include/locomouse_bkg.h): a 256-bin
// histogram of 16-bit counters per pixel in device memory, hist[pixel][256],
// and the value at a rank selected from it (lm_bkg_core.h).
//
//   k_bkg_accum<PX>  one thread owns PX adjacent pixels and their histograms
//                    for the whole launch and walks the batch's frames: no
//                    atomics, and launches are ordered on the context's
//                    stream.  Frame reads are coalesced over the wave (one
//                    dword per lane for PX = 4 when base and pitch are
//                    4-aligned, bytes otherwise and in the last, short group).
//                    Equal consecutive samples of a pixel are counted in
//                    registers and added in one update (LmbRun).
//   k_bkg_select     one thread per pixel: running sum over its 256 counters
//                    until it passes the rank.
//
// Safety: a thread's pixels are [p0, p0 + cnt) with p0 + cnt <= npix, the
// context's rows * cols, which sizes the histogram; frames are read at
// i * pitch + p for i < n only, and pitch >= npix, n <= max_batch and the
// sample cap are checked on the host before anything is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "locomouse_bkg.h"
#include "lm_bkg_core.h"
#include "lm_host.h"

static_assert(LM_BKG_MAX_SAMPLES == LMB_MAX_SAMPLES, "the header's cap is the counters'");
static_assert((lmb_count)LMB_MAX_SAMPLES == LMB_MAX_SAMPLES, "the cap fits a counter");

namespace {

constexpr int kThreads = 256;
constexpr int kAhead = 4;  // frames whose pixels are loaded before their updates begin

template <int PX>
__global__ __launch_bounds__(kThreads) void k_bkg_accum(const uint8_t* __restrict__ frames, int64_t pitch, int n,
                                                        uint32_t npix, int vec, lmb_count* hist) {
  const uint64_t p0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * PX;
  if (p0 >= npix) return;
  const int cnt = npix - p0 < (uint64_t)PX ? (int)(npix - p0) : PX;
  const bool whole = vec && cnt == PX;
  lmb_count* h = hist + p0 * LMB_BINS;
  const uint8_t* src = frames + p0;
  LmbRun run[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) run[k] = LmbRun{0, 0};
  for (int f0 = 0; f0 < n; f0 += kAhead) {
    uint32_t w[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      w[j] = 0;
      if (f0 + j < n) {
        const uint8_t* s = src + (int64_t)(f0 + j) * pitch;
        if (PX == 4 && whole) {
          w[j] = *reinterpret_cast<const uint32_t*>(s);
        } else if (PX == 2 && whole) {
          w[j] = *reinterpret_cast<const uint16_t*>(s);
        } else {
#pragma unroll
          for (int k = 0; k < PX; ++k)
            if (k < cnt) w[j] |= (uint32_t)s[k] << (8 * k);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (f0 + j < n) {
#pragma unroll
        for (int k = 0; k < PX; ++k)
          if (k < cnt) lmb_push(h + k * LMB_BINS, run[k], (w[j] >> (8 * k)) & 255u);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PX; ++k)
    if (k < cnt) lmb_flush(h + k * LMB_BINS, run[k]);
}

__global__ __launch_bounds__(kThreads) void k_bkg_select(const lmb_count* __restrict__ hist, uint32_t npix,
                                                         uint32_t rank, uint8_t* __restrict__ out) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= npix) return;
  out[p] = lmb_select(hist + p * LMB_BINS, rank);
}

}  // namespace

struct lm_bkg_ctx {
  int device = 0;
  int rows = 0, cols = 0, max_batch = 0;
  int px = 4;  // pixels per thread of k_bkg_accum (LM_BKG_PX: 1, 2 or 4; diagnostics)
  uint32_t npix = 0;
  int64_t samples = 0;
  hipStream_t stream = nullptr;
  DevBuf<lmb_count> d_hist;
  DevBuf<uint8_t> d_stage;  // lm_bkg_push: the batch's frames, tightly packed (allocated at the first host push)
  DevBuf<uint8_t> d_out;
  HostBuf<uint8_t> h_out;
  ~lm_bkg_ctx() {
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

void check_push(const lm_bkg_ctx* c, int64_t pitch, int n) {
  if (n < 0 || n > c->max_batch) throw std::invalid_argument("n exceeds the context's max_batch");
  if (pitch < (int64_t)c->npix) throw std::invalid_argument("pitch is smaller than a frame");
  if (c->samples + n > LM_BKG_MAX_SAMPLES)
    throw std::invalid_argument("the push would take the sample count past LM_BKG_MAX_SAMPLES (" +
                                std::to_string(LM_BKG_MAX_SAMPLES) + "): " + std::to_string(c->samples) + " + " +
                                std::to_string(n));
}

void launch_accum(lm_bkg_ctx* c, const uint8_t* d_frames, int64_t pitch, int n) {
  const int vec = ((uintptr_t)d_frames % 4 == 0 && pitch % 4 == 0) ? 1 : 0;
  const uint32_t groups = (c->npix + (uint32_t)c->px - 1) / (uint32_t)c->px;
  const dim3 grid((groups + kThreads - 1) / kThreads), block(kThreads);
  if (c->px == 1)
    hipLaunchKernelGGL(k_bkg_accum<1>, grid, block, 0, c->stream, d_frames, pitch, n, c->npix, vec, c->d_hist.p);
  else if (c->px == 2)
    hipLaunchKernelGGL(k_bkg_accum<2>, grid, block, 0, c->stream, d_frames, pitch, n, c->npix, vec, c->d_hist.p);
  else
    hipLaunchKernelGGL(k_bkg_accum<4>, grid, block, 0, c->stream, d_frames, pitch, n, c->npix, vec, c->d_hist.p);
  HIPCHK(hipGetLastError());
  c->samples += n;
}

}  // namespace

LM_API lm_status lm_bkg_create(int32_t device, int32_t rows, int32_t cols, int32_t max_batch, lm_bkg_ctx** out) {
  if (!out) return fail(LM_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (max_batch <= 0 || max_batch > 65535) return fail(LM_ERR_INVALID_ARGUMENT, "max_batch must be in 1..65535");
  if (rows <= 0 || cols <= 0 || rows > 65535 || cols > 65535)
    return fail(LM_ERR_INVALID_ARGUMENT, "rows and cols must be in 1..65535");
  if ((int64_t)rows * cols > (int64_t)1 << 25) return fail(LM_ERR_INVALID_ARGUMENT, "frame too large");
  int px = 4;
  if (const char* v = getenv("LM_BKG_PX")) {
    px = atoi(v);
    if (px != 1 && px != 2 && px != 4) return fail(LM_ERR_INVALID_ARGUMENT, "LM_BKG_PX must be 1, 2 or 4");
  }
  lm_bkg_ctx* c = new lm_bkg_ctx();
  lm_status s = guarded([&] {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw HipError("invalid HIP device index");
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->rows = rows;
    c->cols = cols;
    c->max_batch = max_batch;
    c->px = px;
    c->npix = (uint32_t)rows * (uint32_t)cols;
    c->d_hist.alloc((size_t)c->npix * LMB_BINS);
    c->d_out.alloc(c->npix);
    c->h_out.alloc(c->npix);
    SET_SYNC(c->d_hist.p, 0, sizeof(lmb_count) * LMB_BINS * (size_t)c->npix, c->stream);
  });
  if (s != LM_OK) {
    delete c;
    return s;
  }
  *out = c;
  return LM_OK;
}

LM_API void lm_bkg_destroy(lm_bkg_ctx* ctx) { delete ctx; }

LM_API lm_status lm_bkg_push(lm_bkg_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n) {
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
    launch_accum(ctx, ctx->d_stage.p, (int64_t)fb, n);
  });
}

LM_API lm_status lm_bkg_push_device(lm_bkg_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n) {
  if (!ctx || !d_frames) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_push(ctx, pitch, n);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    launch_accum(ctx, d_frames, pitch, n);
  });
}

LM_API lm_status lm_bkg_finish(lm_bkg_ctx* ctx, int32_t permille, uint8_t* out) {
  if (!ctx || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (permille < 0 || permille > 1000) return fail(LM_ERR_INVALID_ARGUMENT, "permille must be in 0..1000");
  if (ctx->samples < 1) return fail(LM_ERR_INVALID_ARGUMENT, "no frames were pushed");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t rank = lmb_rank(permille, ctx->samples);
    hipLaunchKernelGGL(k_bkg_select, dim3((ctx->npix + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream,
                       ctx->d_hist.p, ctx->npix, rank, ctx->d_out.p);
    HIPCHK(hipGetLastError());
    COPY_SYNC(ctx->h_out.p, ctx->d_out.p, ctx->npix, hipMemcpyDeviceToHost, ctx->stream);
    std::memcpy(out, ctx->h_out.p, ctx->npix);
  });
}

LM_API lm_status lm_bkg_reset(lm_bkg_ctx* ctx) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    SET_SYNC(ctx->d_hist.p, 0, sizeof(lmb_count) * LMB_BINS * (size_t)ctx->npix, ctx->stream);
    ctx->samples = 0;
  });
}

LM_API int64_t lm_bkg_samples(lm_bkg_ctx* ctx) { return ctx ? ctx->samples : -1; }

LM_API void* lm_bkg_stream(lm_bkg_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
