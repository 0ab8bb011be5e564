/* locomouse_train.h — detector weights trained on the device from labelled
 * patches: the model.yml detectors the reference program only ever loads.
 * Part of liblocomouse_hip.so; statuses and lm_last_error are locomouse_hip.h's.
 *
 * Samples are kh x kw u8 patches p_i in row-major tap order (the order
 * filter2D sums in) with labels y_i in {+1, -1}.  With x_i = p_i / 255 the
 * solver minimises the L2-regularised squared-hinge SVM with a regularised
 * bias (liblinear's -s 2 -B 1)
 *
 *   F(w, b) = 1/2 (|w|^2 + b^2) + sum_i C_{y_i} max(0, 1 - y_i (w . x_i + b))^2
 *
 * by a truncated Newton method in fp64 (conjugate gradients on the active
 * set's Hessian, Armijo backtracking), and hands back  W = w / 255  and
 * rho = -b, so that the detector's score  sum W . p - rho  equals w . x + b.
 * F is 1-strongly convex: |(w, b) - (w*, b*)| <= |grad F(w, b)|.  Every sum
 * has a fixed order that depends on the number of samples and on kh x kw
 * only, so a solve is bit-reproducible. */
#ifndef LOCOMOUSE_TRAIN_H
#define LOCOMOUSE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LM_TRAIN_MAX_SIDE 64            /* kh, kw in 1..64 */
#define LM_TRAIN_MAX_SAMPLES (1 << 22)  /* max_samples in 1..2^22 */

typedef struct lm_train_ctx lm_train_ctx;

typedef struct lm_train_point {
  int32_t frame; /* index into the frames of the call */
  int32_t x, y;  /* column, row in the corrected image (the coordinates of the exported tracks) */
  int32_t label; /* +1 or -1 */
} lm_train_point;

typedef struct lm_train_stats {
  double objective;   /* F at the returned point */
  double grad_norm;   /* |grad F| there */
  double grad_norm0;  /* |grad F(0, 0)| */
  int32_t outer_iters;
  int32_t cg_iters;
  int32_t converged;  /* grad_norm <= eps * grad_norm0 */
  int32_t n_active;   /* samples with y z < 1 at the returned point */
} lm_train_stats;

/* A sample set of at most max_samples patches of kh x kw on HIP device `device`. */
lm_status lm_train_create(int32_t device, int32_t kh, int32_t kw, int32_t max_samples, lm_train_ctx** out);
void lm_train_destroy(lm_train_ctx* ctx);

/* Adds n patches (n x kh*kw bytes, host) with labels +1 / -1.  An add that
 * would pass max_samples, or that holds another label, is refused whole
 * (LM_ERR_INVALID_ARGUMENT): nothing is added. */
lm_status lm_train_add_patches(lm_train_ctx* ctx, const uint8_t* patches, const int8_t* labels, int32_t n);

/* Cuts one patch per point from the frames exactly as the detection context
 * `det` reads them: tap (i, j) of point (frame, x, y) is
 * I_PAD[pad_pre_rows + y - kh/2 + i][pad_pre_cols + x - kw/2 + j], that is the
 * frame after the background subtraction, the per-frame normalisation (with
 * the TM methods' imadjust), the calibration gather and the flip, and 0
 * outside the corrected image.  Frame i is at frames + i * pitch, video_rows x
 * video_cols u8 (host memory, or device memory in the layout of
 * lm_detect_submit_device); det must be on the same device.  A context with
 * transform_gray_values on, a frame index outside 0..n_frames-1, a point
 * outside the corrected image, a label other than +1 / -1 and an overfull add
 * are refused whole with LM_ERR_INVALID_ARGUMENT before anything is launched. */
lm_status lm_train_gather(lm_train_ctx* ctx, lm_ctx* det, const uint8_t* frames, int64_t pitch, int32_t n_frames,
                          const lm_train_point* points, int32_t n_points);
lm_status lm_train_gather_device(lm_train_ctx* ctx, lm_ctx* det, const uint8_t* d_frames, int64_t pitch,
                                 int32_t n_frames, const lm_train_point* points, int32_t n_points);

lm_status lm_train_samples(lm_train_ctx* ctx, int32_t* n_pos, int32_t* n_neg);
lm_status lm_train_reset(lm_train_ctx* ctx); /* forget every sample */

/* Samples first .. first + n - 1 as they are stored: n x kh*kw bytes and n labels (either may be NULL). */
lm_status lm_train_patches(lm_train_ctx* ctx, int32_t first, int32_t n, uint8_t* out_patches, int8_t* out_labels);

/* Minimises F with costs c_pos, c_neg > 0 from (0, 0) until
 * |grad F| <= eps * |grad F(0, 0)| or max_iter outer iterations (then LM_OK
 * with stats->converged = 0).  out_W: kh * kw doubles, row-major.  Fails with
 * LM_ERR_INVALID_ARGUMENT on an empty context, a non-positive or non-finite
 * c_pos, c_neg or eps, or max_iter < 0.  One class alone is allowed. */
lm_status lm_train_solve(lm_train_ctx* ctx, double c_pos, double c_neg, double eps, int32_t max_iter, double* out_W,
                         double* out_rho, lm_train_stats* stats);

/* ---- several problems on the same samples in one pass (cross-validation of the costs).
 *
 * Problem p minimises F with its own costs and with C_i = 0 for the samples of
 * its held-out group.  There is one solver: lm_train_solve is the call of the
 * one problem {c_pos, c_neg, held_out = -1}, so starting point, stopping rule,
 * the CG tolerance and cap, the line search and the scaling of W and rho are
 * the same.  Within one problem every sum is taken in an order that depends on
 * the samples alone (a sample of cost 0 adds +-0), so any problem returns the
 * same, to the bit, alone or in any company and order. */
#define LM_TRAIN_MAX_PROBLEMS 64
#define LM_TRAIN_MAX_GROUPS 256

typedef struct lm_train_problem {
  double c_pos, c_neg; /* > 0, finite */
  int32_t held_out;    /* a group whose samples get cost 0 in F, or -1: none */
  int32_t reserved;    /* 0 */
} lm_train_problem;

typedef struct lm_train_heldout { /* of the held-out group, at the returned point, from the solver's own z */
  int32_t n_pos, n_neg;           /* its samples by label */
  int32_t miss_pos, miss_neg;     /* positives with z <= 0, negatives with z > 0 */
} lm_train_heldout;

/* Gives stored sample i the group groups[i] in 0..LM_TRAIN_MAX_GROUPS-1; n must
 * be the number of stored samples.  A later lm_train_add_patches,
 * lm_train_gather or lm_train_reset forgets the groups. */
lm_status lm_train_set_groups(lm_train_ctx* ctx, const int32_t* groups, int32_t n);

/* Solves n_problems (1..LM_TRAIN_MAX_PROBLEMS) problems.  out_W: n_problems x
 * kh*kw doubles, out_rho: n_problems; stats and heldout (n_problems each) may
 * be NULL.  A held-out group without samples is allowed (counts 0), and so is
 * one that leaves a single class.  Refused with LM_ERR_INVALID_ARGUMENT before
 * any launch: what lm_train_solve refuses, n_problems out of range, a cost
 * that is not positive and finite, reserved != 0, held_out outside -1..255,
 * held_out >= 0 while no groups are set, and a held-out group that holds every
 * stored sample. */
lm_status lm_train_solve_many(lm_train_ctx* ctx, const lm_train_problem* problems, int32_t n_problems, double eps,
                              int32_t max_iter, double* out_W, double* out_rho, lm_train_stats* stats,
                              lm_train_heldout* heldout);

/* Problems that share one pass over the sample matrix at this kh x kw; more run as several blocks. */
int32_t lm_train_problem_block(lm_train_ctx* ctx);

/* z_i = sum W . p_i - rho of any model on the stored samples (out_z: one double per sample). */
lm_status lm_train_margins(lm_train_ctx* ctx, const double* W, double rho, double* out_z);

void* lm_train_stream(lm_train_ctx* ctx); /* hipStream_t of the kernels */

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_TRAIN_H */
