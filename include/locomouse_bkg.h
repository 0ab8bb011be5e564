/* locomouse_bkg.h — the video's background estimated on the device as the
 * per-pixel temporal median (or any other rank) of its channel-0 frames: the
 * background.png the reference program only ever loads.  Part of
 * liblocomouse_hip.so; statuses and lm_last_error are locomouse_hip.h's.
 *
 * For K pushed frames and permille in 0..1000, each pixel of the result is the
 * value at zero-based index  rank = (permille * (K - 1)) / 1000  (64-bit
 * integer arithmetic) of that pixel's K samples sorted ascending; permille
 * 500 is the lower median.  No floating point is used.
 *
 * The state is a 256-bin histogram of 16-bit counters per pixel in device
 * memory (512 bytes per pixel: 134 MB at 1024 x 256, 503 MB at 1920 x 512),
 * so K is bounded by the counters, not by memory: LM_BKG_MAX_SAMPLES.  A pixel
 * the animal covers in more than half of the pushed frames comes out as
 * animal, not as background. */
#ifndef LOCOMOUSE_BKG_H
#define LOCOMOUSE_BKG_H

#include <stddef.h>
#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LM_BKG_MAX_SAMPLES 65535 /* frames one context accumulates (16-bit counters) */

typedef struct lm_bkg_ctx lm_bkg_ctx;

/* An estimator for frames of rows x cols, at most max_batch (1..65535) per
 * push, on HIP device `device`. */
lm_status lm_bkg_create(int32_t device, int32_t rows, int32_t cols, int32_t max_batch, lm_bkg_ctx** out);
void lm_bkg_destroy(lm_bkg_ctx* ctx);

/* Adds n <= max_batch frames: frame i at base + i * pitch, rows x cols u8,
 * row-major, pitch >= rows * cols (the layout of lm_detect_submit_device,
 * lm_bb_push_device and lm_jpeg_decode_device).  lm_bkg_push takes host memory
 * (page-locked memory from lm_host_alloc is copied by DMA) and returns once
 * the frames are copied; lm_bkg_push_device takes device memory, which must
 * stay valid and unchanged until the context's stream has passed the push
 * (lm_bkg_finish waits for it).  A push that would take the sample count past
 * LM_BKG_MAX_SAMPLES is refused whole (LM_ERR_INVALID_ARGUMENT): nothing is
 * accumulated. */
lm_status lm_bkg_push(lm_bkg_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n);
lm_status lm_bkg_push_device(lm_bkg_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n);

/* The image at `permille` (0..1000) of the frames pushed so far into out
 * (rows * cols bytes, host).  The accumulated state is kept: it can be asked
 * again with another permille, and pushes may continue.  Fails with
 * LM_ERR_INVALID_ARGUMENT when nothing was pushed. */
lm_status lm_bkg_finish(lm_bkg_ctx* ctx, int32_t permille, uint8_t* out);

lm_status lm_bkg_reset(lm_bkg_ctx* ctx);  /* forget every pushed frame */
int64_t lm_bkg_samples(lm_bkg_ctx* ctx);  /* frames accumulated so far (-1: ctx is NULL) */
void* lm_bkg_stream(lm_bkg_ctx* ctx);     /* hipStream_t of the kernels */

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_BKG_H */
