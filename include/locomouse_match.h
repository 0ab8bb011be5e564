/* locomouse_match.h — every frame's bottom crop matched to a reference
 * image's histogram: what use_reference_image_brightness intends
 * (cropBoundingBox, LocoMouse_class.cpp:1437-1443; histogramMatching,
 * :3313-3387; computeNormalizedCDF, :3389-3414).  The reference cannot start
 * with that option, and lm_ctx_create fails with it as the reference does; a
 * matched context is asked for here, by name.  Part of liblocomouse_hip.so;
 * statuses and lm_last_error are locomouse_hip.h's.
 *
 * Per frame: h[256] counts the corrected pixels (background subtraction, the
 * frame's normalisation table, the calibration gather and the flip) of the
 * bottom box I_BOTTOM_MOUSE, n = height * width of them;
 *   p[i] = (float)h[i] * (float)(1.0 / (double)n),
 *   c[0] = p[0], c[i] = c[i - 1] + p[i]  (float, in index order);
 * the table T is the reference's two loops: cur = 0; for i = 0..255 the first
 * j >= cur with ref[j] >= c[i] gives T[i] = cur = j; if there is none,
 * min_diff = 1.0f and j = cur..255 updates (min_diff, cur) wherever
 * c[i] - ref[j] < min_diff, then T[i] = cur.  T replaces the pixels of the
 * frame's box for the rest of that frame, and in I_PREV_PAD for the next. */
#ifndef LOCOMOUSE_MATCH_H
#define LOCOMOUSE_MATCH_H

#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cumulative histogram c[256] (above) of a rows x cols u8 image, row r at
 * image + r * pitch (pitch >= cols), with n = rows * cols.  Host only; no
 * device is touched. */
lm_status lm_match_cdf(const uint8_t* image, int32_t rows, int32_t cols, int64_t pitch, float out_cdf[256]);

/* lm_ctx_create with every frame's bottom crop matched to reference_cdf: 256
 * finite, non-negative, non-decreasing floats (lm_match_cdf of the reference
 * image).  params->use_reference_image_brightness and
 * params->transform_gray_values must both be 0 (LM_ERR_INVALID_ARGUMENT
 * otherwise); everything else is lm_ctx_create's.  A batch with a frame whose
 * bottom box leaves the corrected image is refused before anything is
 * launched (LM_ERR_INVALID_ARGUMENT), and lm_train_gather refuses a matched
 * context. */
lm_status lm_ctx_create_matched(int32_t device, const lm_setup* setup, const lm_params* params, const lm_model* model,
                                const float reference_cdf[256], int32_t max_batch, lm_ctx** out);

/* Of frame f (0-based) of the last collected batch of a matched context, while
 * its lane still holds it: the histogram, the table, and the bottom box (rows
 * x cols = its height x width) as frame f's steps see it -- prev = 0: the
 * current image; prev = 1: I_PREV_PAD at the current box (the frame before,
 * with its own table inside its own box).  The crop is read through the
 * accessor the kernels use; the batch's frames must still be where they were
 * when it ran (always, for host frames). */
lm_status lm_debug_match_hist(lm_ctx* ctx, int32_t f, uint32_t out[256]);
lm_status lm_debug_match_table(lm_ctx* ctx, int32_t f, uint8_t out[256]);
lm_status lm_debug_match_crop(lm_ctx* ctx, int32_t f, int32_t prev, uint8_t* out, int32_t rows, int32_t cols);

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_MATCH_H */
