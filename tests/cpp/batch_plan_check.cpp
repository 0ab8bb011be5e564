// batch_plan_check.cpp — the host's plan of a submitted batch (csrc/
// lm_batch_plan.h: the continuation mode, the slot table with its two bounds
// rules, the inherited corners, the source-map decision) against the
// reference's per-frame loop, on the host: a plain program, also built with
// -fsanitize=address,undefined by tests/test_batch_plan.py.
//
// The definition it checks against is not the runtime's slot loop but the
// reference's frame loop (main.cpp:54-82: every frame is read and cropped
// once, cropBoundingBox :1408-1478): every video frame g has ONE set of
// corners, the ones the caller passed for g when g was first submitted (its
// bb row, row 0 of a shard start's halo, or the provided box without bb), and
// its crops are cropBoundingBox's formula on those corners, wherever and how
// often the frame turns up in a slot.
//
// Seeded scripts of submissions drive the header the way submit_batch does
// (lm_bp_continues, a simulated lane pick, lm_bp_mode, lm_bp_slots,
// lm_bp_uniform_crop, then the runtime's advance of the context and the lane)
// over 1 to 4 lanes, batch sizes 1 .. B with a ragged last batch, starts at
// frame 0 and shard starts, bb given or not per batch, picks of the continuing
// lane and of another one, failed batches that clear a lane's state, frame
// gaps and refused crops.  The checker keeps its own books next to the
// simulated context: which lane ran the previous batch and whether anything
// happened there since, every frame's corners, and how often each frame was
// processed.
//
// Prints
//   <n> scripts, <b> batches, <s> slots, modes first <a> given <b> carry <c> handoff <d>, refused roi_bottom <e>
//   roi_side <f> lut <g> gap <h> failed <i>, views uniform <j> nonuniform <k>, carried slot0 <l>, <c> checks, <f> failures
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

struct Tally {
  long scripts = 0, batches = 0, slots = 0, first = 0, given = 0, carry = 0, handoff = 0;
  long roi_b = 0, roi_s = 0, lut = 0, gap = 0, failed = 0, uni = 0, nonuni = 0, carried0 = 0, checks = 0, fails = 0;
};
Tally T;
std::string g_where;

void check(bool ok, const char* what, long a = 0, long b = 0) {
  ++T.checks;
  if (!ok && T.fails++ < 20) std::printf("FAIL %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
}

const char* kGapText = "frame first_frame-1 was not processed by this context: pass prev_frame (shard start).";
const char* kFailedText = "the previous batch failed: pass prev_frame to continue from frame first_frame.";

struct Corners {
  int x, yb, ys;
  bool operator==(const Corners& o) const { return x == o.x && yb == o.yb && ys == o.ys; }
};

// A setting: the geometry fields the crop formula and the bounds rules read
// (as LocoMouse::LocoMouse :307-345 and LocoMouse_Model :3157-3173 derive them
// from the image, the two provided boxes and the largest point detector per
// view), the provided box's corners and how far the scripts move the corners.
struct Setting {
  const char* name;
  lm_geometry g;
  Corners box;
  int ax, ayb, ays;
};

Setting make_setting(const char* name, int rows, int cols, lm_rect ub, lm_rect us, int mtb, int mts, int ax, int ayb,
                     int ays) {
  Setting S{};
  S.name = name;
  lm_geometry& g = S.g;
  g.n_rows = rows;
  g.n_cols = cols;
  g.spre_b_w = g.spre_b_h = mtb / 2;  // ceil((m - 1) / 2)
  g.spre_t_w = g.spre_t_h = mts / 2;
  g.spost_b_w = g.spost_b_h = g.spre_b_w;  // (:3173: the bottom view's post size is its pre size)
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
  S.box = Corners{ub.x + ub.width, ub.y + ub.height, us.y + us.height};
  S.ax = ax;
  S.ayb = ayb;
  S.ays = ays;
  return S;
}

// ---- the definition: one frame's crops from its corners (cropBoundingBox)
struct Crops {
  int x[2], y[2];
};
Crops def_crops(const lm_geometry& g, Corners c) {
  const unsigned bx = (unsigned)c.x, byb = (unsigned)c.yb, bys = (unsigned)c.ys;  // (the reference's corners are unsigned)
  const unsigned pc = (unsigned)g.pad_pre_cols, pr = (unsigned)g.pad_pre_rows;
  Crops R;
  R.x[0] = (int)((bx + pc) - (unsigned)(g.bb_bottom_mouse_pad.width - g.spost_b_w) + 1);
  R.y[0] = (int)((byb + pr) - (unsigned)(g.bb_bottom_mouse_pad.height - g.spost_b_h) + 1);
  R.x[1] = (int)((pc + bx) - (unsigned)(g.bb_side_mouse_pad.width - g.spost_t_w) + 1);
  R.y[1] = (int)((pr + bys) - (unsigned)(g.bb_side_mouse_pad.height - g.spost_t_h) + 1);
  return R;
}
bool inside(int x, int y, int w, int h, int x0, int y0, int x1, int y1) {  // [x, x + w) x [y, y + h) in [x0, x1) x [y0, y1)
  return x >= x0 && y >= y0 && x + w <= x1 && y + h <= y1;
}
bool def_roi_ok(const lm_geometry& g, const Crops& R, int v) {  // the padded crop in I_PAD
  const lm_rect& P = v ? g.bb_side_mouse_pad : g.bb_bottom_mouse_pad;
  return inside(R.x[v], R.y[v], P.width, P.height, 0, 0, g.ipad_cols, g.ipad_rows);
}
bool def_lut_ok(const lm_geometry& g, const Crops& R) {  // the bottom crop without its pads in the corrected image
  return inside(R.x[0] + g.spre_b_w, R.y[0] + g.spre_b_h, g.bb_bottom_mouse.width, g.bb_bottom_mouse.height,
                g.pad_pre_cols, g.pad_pre_rows, g.pad_pre_cols + g.n_cols, g.pad_pre_rows + g.n_rows);
}

// ---- scripts
struct Rng {
  uint64_t s;
  unsigned next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(s >> 33);
  }
  int upto(int n) { return (int)(next() % (unsigned)n); }  // 0 .. n - 1
  bool chance(int percent) { return upto(100) < percent; }
};

struct SimLane {
  bool have_state = false;
  int last_frame = -1;
};
struct Sim {  // what submit_batch reads of the context and its lanes, and advances after a launch
  std::vector<SimLane> lanes;
  bool have_state = false;
  int last_frame = -1, last_lane = -1;
  int last_bb[3] = {0, 0, 0};
};
struct Books {  // the checker's own
  int last = -2;             // the last frame of the previous batch (-2: none yet)
  int prev_lane = -1;        // the lane that ran the previous batch
  bool prev_intact = false;  // nothing ran or failed there since
  std::map<int, Corners> corners;
  std::map<int, int> processed;  // frame -> times processed in a slot >= 1
  long slot0_processed = 0, later_not_carried = 0;
};

Corners moved(const Setting& S, int g) {
  return Corners{S.box.x + (g * 7) % (2 * S.ax + 1) - S.ax, S.box.yb + (g * 5) % (2 * S.ayb + 1) - S.ayb,
                 S.box.ys + (g * 3) % (2 * S.ays + 1) - S.ays};
}

// One submission of frames [first, first + n); returns whether it was accepted.
// safe: the frames' corners are the box's (the retry after a refused crop).
bool submit(const Setting& S, bool gray, Sim& C, Books& K, Rng& R, int first, int n, bool prev_given, bool with_bb,
            bool safe) {
  const lm_geometry& g = S.g;
  const int nl = (int)C.lanes.size();
  ++T.batches;
  // -- continuation (before the lane is picked)
  const bool exp_given = prev_given && first > 0, exp_cont = !exp_given && first > 0;
  bool cont = false;
  try {
    cont = lm_bp_continues(first, prev_given, C.have_state, C.last_frame);
    check(!exp_cont || K.last == first - 1, "a frame gap was accepted", first, K.last);
  } catch (const std::invalid_argument& e) {
    check(exp_cont && K.last != first - 1, "a continuation was refused", first, K.last);
    check(std::string(e.what()) == kGapText, "the frame gap's text");
    ++T.gap;
    return false;
  }
  check(cont == exp_cont, "cont", cont, exp_cont);
  // -- the lane pick: the continuing lane (as acquire_lane prefers) or, as if it were busy, another one
  const int from = cont ? first - 1 : -2;
  int cont_lane = -1;
  for (int l = 0; l < nl; ++l) {
    const bool yes = lm_bp_lane_continues(l, C.lanes[l].have_state, C.lanes[l].last_frame, C.last_lane, from);
    check(yes == (cont && l == K.prev_lane && K.prev_intact), "the lane's answer to 'continues'", l, yes);
    if (yes) cont_lane = l;
  }
  int pick = R.upto(nl);
  if (cont_lane >= 0 && R.chance(60)) pick = cont_lane;
  const bool exp_carry = cont && pick == K.prev_lane && K.prev_intact, exp_handoff = cont && !exp_carry;
  // -- mode
  LmBatchMode M{};
  try {
    M = lm_bp_mode(first, prev_given, cont, pick == cont_lane, nl > 1);
    check(!(exp_handoff && nl == 1), "a hand-off on a one-lane context was accepted");
  } catch (const std::invalid_argument& e) {
    check(exp_handoff && nl == 1, "a mode was refused", first, pick);
    check(std::string(e.what()) == kFailedText, "the failed batch's text");
    ++T.failed;
    return false;
  }
  check(M.given_halo == exp_given && M.cont == exp_cont && M.carry == exp_carry && M.handoff == exp_handoff, "mode flags");
  check(M.halo == (exp_given || exp_handoff), "halo", M.halo);
  check((M.s_lut0 == 0) == (first > 0) && (M.s_lut0 == 0 || M.s_lut0 == 1), "s_lut0 == 0 iff first > 0", M.s_lut0, first);
  check((M.s_proc0 == 0) == (exp_given || exp_handoff) && (M.s_proc0 == 0 || M.s_proc0 == 1),
        "s_proc0 == 0 iff the batch has a halo", M.s_proc0);
  const int s_lut0 = first > 0 ? 0 : 1, s_proc0 = (exp_given || exp_handoff) ? 0 : 1;
  // -- what the caller passes: every frame's corners by the definition, then the rows of bb
  std::vector<Corners> want((size_t)n + 1, S.box);  // per slot
  if (s_lut0 == 0) {
    const auto it = K.corners.find(first - 1);
    if (it != K.corners.end()) want[0] = it->second;  // seen before: its corners stay
    else if (with_bb && !safe) want[0] = moved(S, first - 1);
    check(exp_given || it != K.corners.end(), "the definition lacks the continued frame", first - 1);
    if (exp_given && !(want[0] == S.box)) with_bb = true;  // (a halo's corners reach the runtime only through bb)
  }
  for (int s = 1; s <= n; ++s)
    if (with_bb && !safe) want[s] = moved(S, first - 1 + s);
  std::vector<int32_t> rows(3 + 3 * ((size_t)n + 1), 0x5a5a5a);  // (three words in front: a wrong row index stays inside)
  int32_t* bb = rows.data() + 3;
  for (int s = exp_given ? 0 : 1; s <= n; ++s) {
    int32_t* r = bb + 3 * (exp_given ? s : s - 1);
    r[0] = want[s].x, r[1] = want[s].yb, r[2] = want[s].ys;
  }
  // -- the definition's verdict, in the frame loop's order: crop (ROI), then the LUT
  int exp_fail = 0;  // 1 ROI bottom, 2 ROI side, 3 LUT
  int fail_frame = -1;
  for (int s = s_lut0; s <= n && !exp_fail; ++s) {
    const Crops D = def_crops(g, want[s]);
    if (s >= s_proc0 && !def_roi_ok(g, D, 0)) exp_fail = 1;
    else if (s >= s_proc0 && !def_roi_ok(g, D, 1)) exp_fail = 2;
    else if (gray && !def_lut_ok(g, D)) exp_fail = 3;
    if (exp_fail) fail_frame = first - 1 + s;
  }
  // -- the slot table
  std::vector<LmSlot> slots((size_t)n + 1);
  std::memset(slots.data(), 0xff, slots.size() * sizeof(LmSlot));
  const int box[3] = {S.box.x, S.box.yb, S.box.ys};
  int new_last[3] = {-1, -1, -1};
  int got_fail = 0;
  std::string text;
  try {
    lm_bp_slots(n, first, M, g, box, gray, with_bb ? bb : nullptr, C.last_bb, slots.data(), new_last);
  } catch (const std::runtime_error& e) {
    text = e.what();
    got_fail = text == "ROI out of image bounds: BB_BOTTOM_MOUSE_PAD" ? 1 : text == "ROI out of image bounds: BB_SIDE_MOUSE_PAD" ? 2 : -1;
  } catch (const std::invalid_argument& e) {
    text = e.what();
    got_fail = text == "transform_gray_values: frame " + std::to_string(fail_frame) +
                           ": the bottom crop leaves the corrected image, so the in-place LUT would reach I_PAD's zero "
                           "padding (not supported)." ? 3 : -1;
  }
  check(got_fail == exp_fail, "the refusal (0 none, 1 ROI bottom, 2 ROI side, 3 LUT)", got_fail, exp_fail);
  if (exp_fail) {
    ++(exp_fail == 1 ? T.roi_b : exp_fail == 2 ? T.roi_s : T.lut);
    return false;
  }
  if (got_fail) return false;
  for (int s = 0; s <= n; ++s) {
    const LmSlot& L = slots[s];
    ++T.slots;
    check(L.frame == first - 1 + s, "slot frame", L.frame, first - 1 + s);
    if (s < s_lut0) {  // (the first batch's slot 0: no frame -1; nothing but its frame number is set)
      check(L.active == 0 && L.crop_x[0] == 0 && L.crop_x[1] == 0 && L.crop_y[0] == 0 && L.crop_y[1] == 0, "slot 0 of frame 0");
      continue;
    }
    const Crops D = def_crops(g, want[s]);
    check(L.active == 1, "active", s, L.active);
    for (int v = 0; v < 2; ++v) check(L.crop_x[v] == D.x[v] && L.crop_y[v] == D.y[v], "crop", s, v);
  }
  check(new_last[0] == want[n].x && new_last[1] == want[n].yb && new_last[2] == want[n].ys, "new last_bb", first + n - 1);
  // -- the source map: a position iff the processed slots' crops of the view agree
  for (int v = 0; v < 2; ++v) {
    const Crops D0 = def_crops(g, want[s_proc0]);
    bool uni = true;
    for (int s = s_proc0 + 1; s <= n; ++s) {
      const Crops D = def_crops(g, want[s]);
      uni = uni && D.x[v] == D0.x[v] && D.y[v] == D0.y[v];
    }
    const auto at = lm_bp_uniform_crop(slots.data(), n, M.s_proc0, v);
    check(at.has_value() == uni, "uniform view", v, uni);
    if (at && uni) check(at->first == D0.x[v] && at->second == D0.y[v], "the source map's position", v);
    ++(uni ? T.uni : T.nonuni);
  }
  // -- the books, then the context's and the lane's position as submit_batch advances them
  ++(first == 0 ? T.first : exp_given ? T.given : exp_carry ? T.carry : T.handoff);
  if (s_lut0 == 0) K.corners.emplace(first - 1, want[0]);
  for (int s = 1; s <= n; ++s) {
    K.corners.emplace(first - 1 + s, want[s]);
    ++K.processed[first - 1 + s];
  }
  if (s_proc0 == 0) ++K.slot0_processed;
  if (first > 0 && !exp_carry) ++K.later_not_carried;
  K.last = first + n - 1;
  K.prev_lane = pick;
  K.prev_intact = true;
  C.have_state = true;
  C.last_frame = first + n - 1;
  std::memcpy(C.last_bb, new_last, sizeof(new_last));
  C.last_lane = pick;
  C.lanes[pick].have_state = true;
  C.lanes[pick].last_frame = first + n - 1;
  return true;
}

void run_script(const Setting& S, uint64_t seed) {
  Rng R{seed * 0x9e3779b97f4a7c15ull + 12345};
  const int nl = 1 + (int)(seed % 4), B = 1 + R.upto(6);
  const bool gray = (seed / 4) % 2 == 1;
  g_where = std::string(S.name) + " seed " + std::to_string(seed);
  ++T.scripts;
  Sim C;
  C.lanes.resize((size_t)nl);
  Books K;
  int next = R.chance(50) ? 0 : 1 + R.upto(40);  // frame 0 or a shard start
  bool need_prev = next > 0;
  if (need_prev && R.chance(50)) submit(S, gray, C, K, R, next, 1, false, true, false);  // (refused: no prev, no state)
  int left = 12 + R.upto(30);
  bool with_bb = R.chance(50);
  while (left > 0) {
    const int n = std::min(left, 1 + R.upto(B));  // (ragged: the last batch takes what is left)
    if (R.chance(25)) with_bb = !with_bb;
    if (!need_prev && K.prev_lane >= 0 && R.chance(10)) {  // the previous batch failed at collection: its lane forgets
      C.lanes[(size_t)K.prev_lane].have_state = false;
      K.prev_intact = false;
    }
    if (!need_prev && K.prev_lane >= 0 && R.chance(8)) submit(S, gray, C, K, R, next + 1 + R.upto(3), n, false, with_bb, false);  // a gap
    if (!need_prev && K.prev_lane >= 0 && R.chance(8)) {  // a shard start further on
      next += 1 + R.upto(5);
      need_prev = true;
    }
    const bool prev_given = need_prev || (next == 0 && R.chance(20));  // (a prev at frame 0 is ignored)
    bool ok = submit(S, gray, C, K, R, next, n, prev_given, with_bb, false);
    if (!ok && !need_prev && nl == 1 && !K.prev_intact && next > 0) {  // one lane, its state lost: the caller passes prev
      need_prev = true;
      ok = submit(S, gray, C, K, R, next, n, true, with_bb, false);
    }
    if (!ok) ok = submit(S, gray, C, K, R, next, n, need_prev, with_bb, true);  // a refused crop: the box's corners
    check(ok, "the batch was refused with the provided box's corners", next, n);
    if (!ok) return;
    next += n;
    left -= n;
    need_prev = false;
  }
  for (const auto& p : K.processed) check(p.second == 1, "a frame was processed in a slot >= 1 more than once", p.first, p.second);
  check(K.slot0_processed == K.later_not_carried, "a slot 0 is processed exactly in the batches that do not carry",
        K.slot0_processed, K.later_not_carried);
}

// The unprocessed slot 0 of a carry is under the LUT rule but not the ROI
// rule.  No script gets there with a crop outside I_PAD (its frame passed the
// ROI rule as the last slot of its own batch), so the slot table is asked
// directly: last_bb far outside, no LUT.
void carried_slot0(const Setting& S) {
  g_where = std::string(S.name) + " carried slot 0";
  const LmBatchMode M = lm_bp_mode(5, false, true, true, false);
  check(M.carry && M.s_lut0 == 0 && M.s_proc0 == 1, "a carry's mode");
  const int box[3] = {S.box.x, S.box.yb, S.box.ys}, far[3] = {-40, -40, -40};
  check(!def_roi_ok(S.g, def_crops(S.g, Corners{far[0], far[1], far[2]}), 0), "the carried crop is meant to lie outside");
  LmSlot slots[3];
  int new_last[3];
  try {
    lm_bp_slots(2, 5, M, S.g, box, false, nullptr, far, slots, new_last);
    const Crops D = def_crops(S.g, Corners{far[0], far[1], far[2]});
    check(slots[0].active == 1 && slots[0].crop_x[0] == D.x[0] && slots[0].crop_y[1] == D.y[1], "the carried slot's crop");
    ++T.carried0;
  } catch (const std::exception&) {
    check(false, "the ROI rule was applied to the unprocessed slot 0 of a carry");
  }
}

}  // namespace

int main() {
  const Setting settings[] = {
      make_setting("C3", 256, 1024, lm_rect{300, 106, 400, 140}, lm_rect{300, 3, 400, 90}, 30, 26, 6, 3, 3),
      make_setting("C5", 512, 1920, lm_rect{600, 212, 800, 280}, lm_rect{600, 6, 800, 180}, 60, 52, 12, 2, 2),
      // small boxes near the top left and the bottom right corner: the moving corners push the crops over every edge
      make_setting("top-left", 120, 200, lm_rect{4, 8, 40, 30}, lm_rect{4, 2, 40, 20}, 12, 20, 45, 25, 16),
      make_setting("bottom-right", 120, 200, lm_rect{156, 88, 40, 30}, lm_rect{156, 90, 40, 20}, 12, 20, 10, 16, 16),
  };
  for (const Setting& S : settings) {
    for (uint64_t seed = 0; seed < 200; ++seed) run_script(S, seed);
    carried_slot0(S);
  }
  std::printf("%ld scripts, %ld batches, %ld slots, modes first %ld given %ld carry %ld handoff %ld, refused roi_bottom %ld "
              "roi_side %ld lut %ld gap %ld failed %ld, views uniform %ld nonuniform %ld, carried slot0 %ld, %ld checks, "
              "%ld failures\n",
              T.scripts, T.batches, T.slots, T.first, T.given, T.carry, T.handoff, T.roi_b, T.roi_s, T.lut, T.gap,
              T.failed, T.uni, T.nonuni, T.carried0, T.checks, T.fails);
  return T.fails ? 1 : 0;
}
