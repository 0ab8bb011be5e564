/*
 * lm_batch_plan.h — the host's plan of one submitted batch (plain C++: the
 * host runtime and tests/cpp/batch_plan_check.cpp share it; no HIP call, no
 * context, no lane): how the batch continues the video, which of its slots
 * get a LUT and which are processed, every slot's frame number and crop
 * rectangles (LocoMouse::cropBoundingBox :1408-1478) with the two bounds
 * rules, the corners the next batch inherits, and whether k_ingest's source
 * map can be rebuilt for a view.  submit_batch (lm_runtime.hip) takes every
 * decision from here and keeps the HIP calls and the frame pointers.
 *
 * A batch of n frames [first, first + n) has slots 0 .. n: slot s >= 1 holds
 * frame first - 1 + s, slot 0 the frame before the batch (the halo), which
 *   - does not exist                      (first == 0: the first batch),
 *   - the caller passed                   (given_halo: a shard start),
 *   - the lane still holds, candidates too (carry: it ran the previous batch),
 *   - another lane handed over as pixels  (handoff: it is processed again).
 * The caller's bb holds one row of corners (x, y bottom, y side) per frame it
 * passes: with a given halo row 0 is the halo's and row s slot s's; without
 * one row s - 1 is slot s's, and slot 0 of a continuation takes the corners
 * its frame had in its own batch (last_bb).
 */
#ifndef LM_BATCH_PLAN_H
#define LM_BATCH_PLAN_H

#include <stdint.h>

#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>

#include "lm_device.h"
#include "locomouse_hip.h"

// Lane `lane` continues the video after `frame` with its own state: it ran
// the context's previous batch, which ended with `frame`, and nothing ran
// there since (a batch that failed there cleared lane_have_state).
inline bool lm_bp_lane_continues(int lane, bool lane_have_state, int lane_last_frame, int ctx_last_lane, int frame) {
  return lane == ctx_last_lane && lane_have_state && lane_last_frame == frame;
}

struct LmBatchMode {
  bool given_halo;      // the caller passed frame first - 1
  bool cont;            // frame first - 1 ended the context's previous batch
  bool carry;           // ... on the picked lane: slot 0 carries that batch's candidates (k_carry)
  bool handoff;         // ... on another lane: slot 0 is the handed-over frame, processed again
  bool halo;            // slot 0 is processed (given or handed over)
  int s_lut0, s_proc0;  // the first slot with a LUT / that is processed
};

// Whether the batch continues the context's previous one (before a lane is
// picked: acquire_lane prefers the lane that can carry).  A batch that starts
// inside the video with neither a halo frame nor a predecessor is refused.
inline bool lm_bp_continues(int first, bool prev_given, bool ctx_have_state, int ctx_last_frame) {
  const bool cont = !prev_given && first > 0;
  if (cont && !(ctx_have_state && ctx_last_frame == first - 1))
    throw std::invalid_argument("frame first_frame-1 was not processed by this context: pass prev_frame (shard start).");
  return cont;
}

// The batch's mode once its lane is picked.  lane_continues: the picked
// lane's answer to lm_bp_lane_continues for frame first - 1.  A context of one
// lane has no hand-off: its lane lost its state to a failed batch.
inline LmBatchMode lm_bp_mode(int first, bool prev_given, bool cont, bool lane_continues, bool pipelined) {
  LmBatchMode M{};
  M.given_halo = prev_given && first > 0;
  M.cont = cont;
  M.carry = cont && lane_continues;
  M.handoff = cont && !M.carry;
  if (M.handoff && !pipelined)
    throw std::invalid_argument("the previous batch failed: pass prev_frame to continue from frame first_frame.");
  M.halo = M.given_halo || M.handoff;
  M.s_lut0 = first > 0 ? 0 : 1;
  M.s_proc0 = M.halo ? 0 : 1;
  return M;
}

// cropBoundingBox :1420-1470: the padded crops' top-left corners in I_PAD for
// the corners cr = (x, y bottom, y side).  The reference computes them in
// unsigned arithmetic and converts to int: a corner left of or above its box
// wraps around to a negative coordinate.
inline void lm_bp_crop(const lm_geometry& g, const int* cr, LmSlot& S) {
  S.crop_x[0] = (int)((unsigned)(cr[0] + g.pad_pre_cols) - (unsigned)(g.bb_bottom_mouse_pad.width - g.spost_b_w) + 1u);
  S.crop_y[0] = (int)((unsigned)(cr[1] + g.pad_pre_rows) - (unsigned)(g.bb_bottom_mouse_pad.height - g.spost_b_h) + 1u);
  S.crop_x[1] = (int)((unsigned)(g.pad_pre_cols + cr[0]) - (unsigned)(g.bb_side_mouse_pad.width - g.spost_t_w) + 1u);
  S.crop_y[1] = (int)((unsigned)(g.pad_pre_rows + cr[2]) - (unsigned)(g.bb_side_mouse_pad.height - g.spost_t_h) + 1u);
}

// The ROI rule (cv::Mat's ROI assertion): both padded crops of a processed
// slot lie inside I_PAD.
inline void lm_bp_check_roi(const lm_geometry& g, const LmSlot& S) {
  const int w[2] = {g.bb_bottom_mouse_pad.width, g.bb_side_mouse_pad.width};
  const int h[2] = {g.bb_bottom_mouse_pad.height, g.bb_side_mouse_pad.height};
  for (int v = 0; v < 2; ++v)
    if (S.crop_x[v] < 0 || S.crop_y[v] < 0 || S.crop_x[v] + w[v] > g.ipad_cols || S.crop_y[v] + h[v] > g.ipad_rows)
      throw std::runtime_error(std::string("ROI out of image bounds: ") + (v ? "BB_SIDE_MOUSE_PAD" : "BB_BOTTOM_MOUSE_PAD"));
}

// The in-place-LUT rule: the bottom crop (without its pads) stays inside the
// corrected image I_UNPAD, since the LUT is applied to it in I_PAD and must
// not reach the zero padding (see locomouse_hip.h).
inline void lm_bp_check_lut(const lm_geometry& g, const LmSlot& S) {
  const int ux = S.crop_x[0] + g.spre_b_w, uy = S.crop_y[0] + g.spre_b_h;
  if (ux < g.pad_pre_cols || uy < g.pad_pre_rows || ux + g.bb_bottom_mouse.width > g.pad_pre_cols + g.n_cols ||
      uy + g.bb_bottom_mouse.height > g.pad_pre_rows + g.n_rows)
    throw std::invalid_argument("transform_gray_values: frame " + std::to_string(S.frame) +
                                ": the bottom crop leaves the corrected image, so the in-place LUT would reach "
                                "I_PAD's zero padding (not supported).");
}

// The matched context's rule (locomouse_match.h), lm_bp_check_lut's for the
// same reason: the histogram counts the bottom crop's pixels of the corrected
// image, and the table is applied to them in I_PAD.
inline void lm_bp_check_match(const lm_geometry& g, const LmSlot& S) {
  const int ux = S.crop_x[0] + g.spre_b_w, uy = S.crop_y[0] + g.spre_b_h;
  if (ux < g.pad_pre_cols || uy < g.pad_pre_rows || ux + g.bb_bottom_mouse.width > g.pad_pre_cols + g.n_cols ||
      uy + g.bb_bottom_mouse.height > g.pad_pre_rows + g.n_rows)
    throw std::invalid_argument("use_reference_image_brightness: frame " + std::to_string(S.frame) +
                                ": the bottom crop leaves the corrected image, so its histogram would count "
                                "I_PAD's zero padding and the table would reach it (not supported).");
}

// A matched context's tables: k_match computes one for every slot with a
// normalisation table, slots [*s0, *s0 + count) -- the unprocessed slot 0 of a
// carry too, whose frame is the halo: the table equals what its own batch
// computed from the same frame, corners and background.
inline int lm_bp_match_slots(int n, int s_lut0, int* s0) {
  *s0 = s_lut0;
  return n + 1 - s_lut0;
}
// The slot whose table a reader of slot s's frame uses: the current image
// (prev = false) carries slot s's, I_PREV_PAD slot s - 1's -- inside that
// slot's own rectangle.  -1: no such image (the first frame has no I_PREV_PAD).
inline int lm_bp_match_reader(int s, bool prev, int s_lut0) {
  const int t = prev ? s - 1 : s;
  return t >= s_lut0 ? t : -1;
}

// The slot table of a batch: slots[0 .. n] (frame, active, crops; a slot
// without a LUT keeps its frame number and is otherwise zero) and the corners
// of frame first + n - 1 for the next batch.  box: the provided box's corners,
// for every frame the caller passes no row for; bb: the caller's rows or null;
// last_bb: the corners of frame first - 1 from its own batch (read for slot 0
// of a continuation).  Throws what the reference throws for a crop it cannot
// take; nothing of the context has changed by then.
// The ROI rule holds for the processed slots (>= s_proc0).  The LUT rule
// (and, for a matched context, lm_bp_check_match's in its place)
// holds for every slot with a LUT (>= s_lut0), the unprocessed slot 0 of a
// carry too: that one can never newly fail, since the same frame with the
// same corners passed it as the last slot of its own batch.
inline void lm_bp_slots(int n, int first, const LmBatchMode& M, const lm_geometry& g, const int (&box)[3],
                        bool gray_lut_on, const int32_t* bb, const int (&last_bb)[3], LmSlot* slots,
                        int (&new_last_bb)[3], bool matched = false) {
  std::memcpy(new_last_bb, box, sizeof(box));
  for (int s = 0; s <= n; ++s) {
    LmSlot& S = slots[s];
    std::memset(&S, 0, sizeof(S));
    S.frame = first - 1 + s;
    S.active = s >= M.s_lut0;
    if (!S.active) continue;
    const int* cr = box;
    if (bb && (s > 0 || M.given_halo)) cr = bb + 3 * (M.given_halo ? s : s - 1);
    else if (s == 0 && M.cont) cr = last_bb;  // the previous batch's last frame
    if (s == n) std::memcpy(new_last_bb, cr, sizeof(new_last_bb));
    lm_bp_crop(g, cr, S);
    if (s >= M.s_proc0) lm_bp_check_roi(g, S);
    if (gray_lut_on) lm_bp_check_lut(g, S);
    if (matched) lm_bp_check_match(g, S);
  }
}

// k_ingest's source map of view v is built for one crop position: the position
// (x, y) when every processed slot of the batch has its crop there, else nothing.
inline std::optional<std::pair<int, int>> lm_bp_uniform_crop(const LmSlot* slots, int n, int s_proc0, int v) {
  const LmSlot& S0 = slots[s_proc0];
  for (int s = s_proc0 + 1; s <= n; ++s)
    if (slots[s].crop_x[v] != S0.crop_x[v] || slots[s].crop_y[v] != S0.crop_y[v]) return std::nullopt;
  return std::make_pair((int)S0.crop_x[v], (int)S0.crop_y[v]);
}

#endif  // LM_BATCH_PLAN_H
