// match_plan_check.cpp — the batch plan of a matched context (csrc/
// lm_batch_plan.h: lm_bp_slots with matched = true, lm_bp_check_match,
// lm_bp_match_slots, lm_bp_match_reader) against the per-frame statement of
// locomouse_match.h, on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_match.py.
//
// The statement: every video frame has one set of corners (the ones passed
// when it was first submitted).  Its bottom box is the rectangle
// [x - w + 1, x] x [yb - h + 1, yb] of the corrected image; a frame whose box
// leaves that image is refused, wherever it turns up in a slot (after the ROI
// rule, for a processed slot).  Every frame of a batch gets a table, and so
// does the frame before the batch whenever there is one -- as slot 0, from the
// same corners it had in its own batch, so the table is the same.  The
// current image of slot s reads slot s's table, I_PREV_PAD slot s - 1's.
//
// Prints
//   <b> batches, modes first <a> given <b> carry <c> handoff <d>, refused match <e> roi <f>, <c> checks, <f> failures
// and exits 1 on a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "lm_batch_plan.h"

namespace {

long g_checks = 0, g_fails = 0;
void check(bool ok, const char* what, long a = 0, long b = 0) {
  ++g_checks;
  if (!ok && g_fails++ < 20) std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
}

struct Rng {
  uint64_t s;
  unsigned next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(s >> 33);
  }
  int upto(int n) { return (int)(next() % (unsigned)n); }
};

struct Corners {
  int x, yb, ys;
};

lm_geometry make_geometry(int rows, int cols, lm_rect ub, lm_rect us, int mtb, int mts) {
  lm_geometry g{};
  g.n_rows = rows;
  g.n_cols = cols;
  g.spre_b_w = g.spre_b_h = mtb / 2;
  g.spre_t_w = g.spre_t_h = mts / 2;
  g.spost_b_w = g.spost_b_h = g.spre_b_w;
  g.spost_t_w = g.spost_t_h = (mts - 1) / 2;
  g.pad_pre_rows = std::max(us.height, std::max(g.spre_t_h, g.spre_b_h));
  g.pad_pre_cols = std::max(ub.width, std::max(g.spre_t_w, g.spre_b_w));
  g.pad_post_rows = std::max(g.spost_b_h, g.spost_t_h);
  g.pad_post_cols = std::max(g.spost_b_w, g.spost_t_w);
  g.ipad_rows = g.pad_pre_rows + rows + g.pad_post_rows;
  g.ipad_cols = g.pad_pre_cols + cols + g.pad_post_cols;
  g.bb_bottom_mouse = lm_rect{0, 0, ub.width, ub.height};
  g.bb_side_mouse = lm_rect{0, 0, us.width, us.height};
  g.bb_bottom_mouse_pad = lm_rect{0, 0, g.spre_b_w + ub.width + g.spost_b_w, g.spre_b_h + ub.height + g.spost_b_h};
  g.bb_side_mouse_pad = lm_rect{0, 0, g.spre_t_w + us.width + g.spost_t_w, g.spre_t_h + us.height + g.spost_t_h};
  return g;
}

// the statement's two rules for a frame with corners c
bool box_inside(const lm_geometry& g, Corners c) {
  const int x0 = c.x - g.bb_bottom_mouse.width + 1, y0 = c.yb - g.bb_bottom_mouse.height + 1;
  return x0 >= 0 && y0 >= 0 && c.x < g.n_cols && c.yb < g.n_rows;
}
bool roi_inside(const lm_geometry& g, Corners c) {  // both padded crops in I_PAD
  const int xb = c.x + g.pad_pre_cols - g.spre_b_w - g.bb_bottom_mouse.width + 1;
  const int yb = c.yb + g.pad_pre_rows - g.spre_b_h - g.bb_bottom_mouse.height + 1;
  const int xs = c.x + g.pad_pre_cols - g.spre_t_w - g.bb_side_mouse.width + 1;
  const int ys = c.ys + g.pad_pre_rows - g.spre_t_h - g.bb_side_mouse.height + 1;
  return xb >= 0 && yb >= 0 && xb + g.bb_bottom_mouse_pad.width <= g.ipad_cols &&
         yb + g.bb_bottom_mouse_pad.height <= g.ipad_rows && xs >= 0 && ys >= 0 &&
         xs + g.bb_side_mouse_pad.width <= g.ipad_cols && ys + g.bb_side_mouse_pad.height <= g.ipad_rows;
}

}  // namespace

int main() {
  const lm_rect ub{40, 60, 37, 21}, us{40, 5, 37, 30};
  const lm_geometry g = make_geometry(96, 120, ub, us, 9, 7);
  const Corners box{ub.x + ub.width, ub.y + ub.height, us.y + us.height};
  const int boxa[3] = {box.x, box.yb, box.ys};
  long batches = 0, m_first = 0, m_given = 0, m_carry = 0, m_handoff = 0, r_match = 0, r_roi = 0;
  Rng R{12345};
  for (int script = 0; script < 400; ++script) {
    const int lanes = 1 + R.upto(2), B = 1 + R.upto(6);
    std::map<int, Corners> of;        // every frame's corners, fixed when first submitted
    std::map<int, LmSlot> slot_of;    // and the slot it had as a batch's frame
    int last_frame = -1, last_lane = -1;
    bool have_state = false;
    int last_bb[3] = {0, 0, 0};
    int first = R.upto(3) == 0 ? 5 + R.upto(20) : 0;
    // how far this script moves the corners: mostly inside the image, sometimes out of it
    const int amp = R.upto(4) == 0 ? 70 : 8;
    for (int b = 0; b < 8; ++b) {
      const int n = 1 + R.upto(B);
      const bool prev_given = first > 0 && !(have_state && last_frame == first - 1);
      const bool cont = lm_bp_continues(first, prev_given, have_state, last_frame);
      const int lane = lanes == 1 ? 0 : R.upto(2);
      const bool lane_cont = cont && lane == last_lane;
      const LmBatchMode M = lm_bp_mode(first, prev_given, cont, lane_cont, lanes > 1);
      ++batches;
      m_first += first == 0;
      m_given += M.given_halo;
      m_carry += M.carry;
      m_handoff += M.handoff;
      // the caller's rows: with a given halo row 0 is the halo's
      const int nrows = n + (M.given_halo ? 1 : 0);
      std::vector<int32_t> bb((size_t)3 * nrows);
      for (int r = 0; r < nrows; ++r) {
        const int frame = first + r - (M.given_halo ? 1 : 0);
        if (!of.count(frame)) of[frame] = Corners{box.x + R.upto(2 * amp + 1) - amp, box.yb + R.upto(2 * amp + 1) - amp / 2, box.ys};
        bb[3 * r] = of[frame].x;
        bb[3 * r + 1] = of[frame].yb;
        bb[3 * r + 2] = of[frame].ys;
      }
      // the statement's verdict, slot by slot in order
      int bad_frame = -1;
      bool bad_roi = false;
      for (int s = M.s_lut0; s <= n && bad_frame < 0; ++s) {
        const Corners c = of[first - 1 + s];
        if (s >= M.s_proc0 && !roi_inside(g, c)) {
          bad_frame = first - 1 + s;
          bad_roi = true;
        } else if (!box_inside(g, c)) {
          bad_frame = first - 1 + s;
        }
      }
      std::vector<LmSlot> slots((size_t)n + 1);
      int new_last[3];
      bool thrown = false;
      try {
        lm_bp_slots(n, first, M, g, boxa, false, bb.data(), last_bb, slots.data(), new_last, true);
      } catch (const std::invalid_argument& e) {
        thrown = true;
        ++r_match;
        const std::string want = "use_reference_image_brightness: frame " + std::to_string(bad_frame) + ":";
        check(bad_frame >= 0 && !bad_roi && std::string(e.what()).rfind(want, 0) == 0, "the refusal names the frame", bad_frame);
      } catch (const std::runtime_error&) {
        thrown = true;
        ++r_roi;
        check(bad_frame >= 0 && bad_roi, "an ROI refusal", bad_frame);
      }
      check(thrown == (bad_frame >= 0), "refused exactly when a frame's box leaves the image", first, n);
      if (thrown) {  // the context is unchanged; the script goes on from a shard start
        have_state = false;
        first += n;
        continue;
      }
      // which slots get a table
      int s0 = -1;
      const int cnt = lm_bp_match_slots(n, M.s_lut0, &s0);
      check(s0 == (first > 0 ? 0 : 1) && cnt == n + (first > 0 ? 1 : 0), "a table for every frame and the one before", s0, cnt);
      for (int s = s0; s < s0 + cnt; ++s) {
        const Corners c = of[first - 1 + s];
        check(slots[s].active == 1 && slots[s].frame == first - 1 + s, "the slot's frame", s);
        // the box of the slot is the statement's rectangle
        check(slots[s].crop_x[0] + g.spre_b_w - g.pad_pre_cols == c.x - g.bb_bottom_mouse.width + 1 &&
                  slots[s].crop_y[0] + g.spre_b_h - g.pad_pre_rows == c.yb - g.bb_bottom_mouse.height + 1,
              "the slot's box", s);
        if (s == 0 && slot_of.count(first - 1))  // the same frame, the same box: the same table as in its own batch
          check(slots[0].crop_x[0] == slot_of[first - 1].crop_x[0] && slots[0].crop_y[0] == slot_of[first - 1].crop_y[0],
                "slot 0's box is the one the frame had in its own batch");
        if (s >= 1) slot_of[first - 1 + s] = slots[s];
      }
      // which table each reader uses
      for (int s = 1; s <= n; ++s) {
        const int tc = lm_bp_match_reader(s, false, M.s_lut0), tp = lm_bp_match_reader(s, true, M.s_lut0);
        check(tc == s, "the current image reads its own slot's table", s, tc);
        const int frame = first - 1 + s;
        check(frame == 0 ? tp == -1 : (tp >= s0 && slots[tp].frame == frame - 1), "I_PREV_PAD reads the frame before's", s, tp);
      }
      std::memcpy(last_bb, new_last, sizeof(last_bb));
      have_state = R.upto(8) != 0;  // (sometimes the next batch is a shard start)
      last_frame = first + n - 1;
      last_lane = lane;
      first += n;
    }
  }
  std::printf("%ld batches, modes first %ld given %ld carry %ld handoff %ld, refused match %ld roi %ld, %ld checks, %ld failures\n",
              batches, m_first, m_given, m_carry, m_handoff, r_match, r_roi, g_checks, g_fails);
  return g_fails ? 1 : 0;
}
