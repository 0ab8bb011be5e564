/* locomouse_calib.h — the two-view calibration map estimated from a marker
 * video: the calibration.yml (ind_warp_mapping, view_boxes) the reference
 * program only ever loads.  A marker (a pen tip) is moved through the corridor
 * and seen in both views; the side view's columns are then warped so that the
 * same physical point has the same x in both.  Part of liblocomouse_hip.so;
 * statuses and lm_last_error are locomouse_hip.h's.
 *
 * Frames are rows x cols u8; the side view is rows [0, split_row), the bottom
 * view rows [split_row, rows).  With d = max(0, frame - background) over a
 * view's rectangle, the device fills one lm_calib_record per (frame, view),
 * in integers only:
 *   peak      max d
 *   px, py    frame coordinates of the first position in row-major order that
 *             holds the peak (an all-zero view: its top-left corner)
 *   n_above   #{d > threshold} over the view
 *   n_in, S, Sx, Sy
 *             count, sum of d, of d * column and of d * row over the pixels
 *             with d > threshold inside the window, rows [py - R, py + R] and
 *             columns [px - R, px + R] intersected with the view
 *   clipped   1 when that window reaches outside the view
 *
 * lm_calib_fit and lm_calib_map turn the records into the column warp on the
 * host, in fp64 with a fixed order of operations (csrc/lm_calib_core.h):
 *   - a frame is a sample when both views have peak >= min_peak, n_in >=
 *     min_area, n_above - n_in <= max_stray and clipped == 0; its coordinates
 *     are xb = Sx / S of the bottom view and xs = Sx / S of the side view;
 *   - xs = p(xb), a polynomial of degree 1..3 in t = (xb - cols/2) / (cols/2),
 *     from the normal equations (sums in frame order) solved by Cholesky; one
 *     refit after dropping the samples with |residual| > max_resid;
 *   - refused (LM_ERR_RUNTIME, the count or the range in lm_last_error) when
 *     fewer than 8 * (degree + 1) samples remain or their xb range [lo, hi]
 *     spans less than cols / 4;
 *   - q(c) = p(c) on [lo, hi], continued linearly with p' at the nearer end
 *     outside; m(c) = clamp(floor(q(c) + 0.5), 0, cols - 1), refused when not
 *     non-decreasing; ind_warp_mapping(r, c) = r * cols + m(c) for r <
 *     split_row and r * cols + c below; view_boxes = {0, 0, cols, split_row},
 *     {0, split_row, cols, rows - split_row}.  The corrected image has the
 *     video's size.
 * A warp that depends on the row, lens distortion and finding split_row are
 * not attempted. */
#ifndef LOCOMOUSE_CALIB_H
#define LOCOMOUSE_CALIB_H

#include <stddef.h>
#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LM_CALIB_MAX_FRAMES (1 << 20) /* frames one context keeps records of */
#define LM_CALIB_MAX_RADIUS 4096
#define LM_CALIB_MAX_DEGREE 3

typedef struct lm_calib_opts {
  int32_t threshold; /* 0..255; d > threshold counts (default 40) */
  int32_t radius;    /* R, 0..LM_CALIB_MAX_RADIUS (12) */
  int32_t min_peak;  /* 0..255 (80) */
  int32_t min_area;  /* >= 1 (12) */
  int32_t max_stray; /* >= 0 (8) */
  int32_t reserved;  /* 0 */
} lm_calib_opts;

typedef struct lm_calib_record {
  int32_t peak, px, py;
  int32_t n_above, n_in, clipped;
  int64_t S, Sx, Sy;
} lm_calib_record; /* 48 bytes */

typedef struct lm_calib_fit_result {
  int32_t n_frames;  /* frames given */
  int32_t n_samples; /* frames that are samples */
  int32_t n_used;    /* samples the refit kept */
  int32_t degree;
  double rms, max_abs_resid; /* of the refit over its samples, in pixels */
  double lo, hi;             /* xb range of those samples */
  double coef[LM_CALIB_MAX_DEGREE + 1]; /* p(t) = coef[0] + coef[1] t + ...; unused ones 0 */
} lm_calib_fit_result;

typedef struct lm_calib_ctx lm_calib_ctx;

/* The defaults above. */
void lm_calib_default_opts(lm_calib_opts* out);

/* A detector for frames of rows x cols (rows * cols < 2^31) split at
 * split_row (1 <= split_row < rows), at most max_batch (1..65535) per push, on
 * HIP device `device`.  opts NULL: the defaults.  The background starts all
 * zero. */
lm_status lm_calib_create(int32_t device, int32_t rows, int32_t cols, int32_t split_row, int32_t max_batch,
                          const lm_calib_opts* opts, lm_calib_ctx** out);
void lm_calib_destroy(lm_calib_ctx* ctx);

/* The background (rows * cols bytes, host) subtracted from the frames pushed
 * after this call; records of earlier pushes stay as they are. */
lm_status lm_calib_set_background(lm_calib_ctx* ctx, const uint8_t* h_bkg);

/* Appends the records of n <= max_batch frames: frame i at base + i * pitch,
 * rows x cols u8, row-major, pitch >= rows * cols of any alignment (the layout
 * of lm_bkg_push*).  lm_calib_push takes host memory (page-locked memory from
 * lm_host_alloc is copied by DMA) and returns once the frames are copied;
 * lm_calib_push_device takes device memory, which must stay valid and
 * unchanged until the context's stream has passed the push (lm_calib_read
 * waits for it).  A push that would take the frame count past
 * LM_CALIB_MAX_FRAMES is refused whole (LM_ERR_INVALID_ARGUMENT). */
lm_status lm_calib_push(lm_calib_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n);
lm_status lm_calib_push_device(lm_calib_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n);

int64_t lm_calib_frames(lm_calib_ctx* ctx); /* frames pushed so far (-1: ctx is NULL) */

/* Waits for the stream and copies the records of frames first .. first + n - 1
 * to out[n][2] (host): side view, then bottom view. */
lm_status lm_calib_read(lm_calib_ctx* ctx, int64_t first, int32_t n, lm_calib_record* out);

lm_status lm_calib_reset(lm_calib_ctx* ctx); /* forget every pushed frame; the background stays */
void* lm_calib_stream(lm_calib_ctx* ctx);    /* hipStream_t of the kernels */

/* The fit of records[n_frames][2] (side, bottom) described above; touches no
 * device.  opts NULL: the defaults.  degree 1..3, max_resid > 0. */
lm_status lm_calib_fit(const lm_calib_record* records, int32_t n_frames, int32_t rows, int32_t cols, int32_t split_row,
                       const lm_calib_opts* opts, int32_t degree, double max_resid, lm_calib_fit_result* result);

/* ind_warp_mapping (map_out, rows * cols int32) and view_boxes
 * (view_boxes_out, 2 x 4 int32: x, y, width, height of the side and the bottom
 * view) of a fit; touches no device. */
lm_status lm_calib_map(const lm_calib_fit_result* result, int32_t rows, int32_t cols, int32_t split_row,
                       int32_t* map_out, int32_t* view_boxes_out);

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_CALIB_H */
