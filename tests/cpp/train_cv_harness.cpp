// train_cv_harness.cpp — for ctypes (tests/train_cv_harness.py; links the host
// library, makes no GPU call): host/Train.hpp's pure host functions of the
// cross-validation (the LM_TRAIN_CV parser, the fold assignment, the selection
// rule, the check of the labels against the folds) and csrc/lm_train_core.h's
// host statement with a held-out group.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "Train.hpp"
#include "lm_train_core.h"

using namespace locomouse;

extern "C" {

int thc_problem_block(int D) { return lmt_problem_block(D); }
int thc_max_problems() { return LM_TRAIN_MAX_PROBLEMS; }
int thc_max_groups() { return LM_TRAIN_MAX_GROUPS; }

// sizeof and the field offsets of lm_train_problem (0) and lm_train_heldout (1) into out; returns the field count
int thc_layout(int which, int* out) {
  if (which == 0) {
    const int v[] = {(int)sizeof(lm_train_problem), (int)offsetof(lm_train_problem, c_pos),
                     (int)offsetof(lm_train_problem, c_neg), (int)offsetof(lm_train_problem, held_out),
                     (int)offsetof(lm_train_problem, reserved)};
    std::memcpy(out, v, sizeof(v));
    return 4;
  }
  const int v[] = {(int)sizeof(lm_train_heldout), (int)offsetof(lm_train_heldout, n_pos),
                   (int)offsetof(lm_train_heldout, n_neg), (int)offsetof(lm_train_heldout, miss_pos),
                   (int)offsetof(lm_train_heldout, miss_neg)};
  std::memcpy(out, v, sizeof(v));
  return 4;
}

// out: folds, the number of scales, then the scales (cap doubles in all); returns 1 with the parser's message in msg
int thc_parse_cv(const char* spec, double* out, int cap, char* msg, int msg_cap) {
  TrainOptions o;
  try {
    parse_train_cv_spec(spec, o);
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)msg_cap, "%s", e.what());
    return 1;
  }
  out[0] = o.cv_folds;
  out[1] = (double)o.cv_scales.size();
  for (size_t k = 0; k < o.cv_scales.size() && (int)k + 2 < cap; ++k) out[k + 2] = o.cv_scales[k];
  return 0;
}

void thc_folds(const int* sample_frames, int n, int folds, int32_t* out) {
  const std::vector<int32_t> f = cv_fold_of_samples(std::vector<int>(sample_frames, sample_frames + n), folds);
  std::memcpy(out, f.data(), sizeof(int32_t) * f.size());
}

// rows: n x (n_pos, n_neg, miss_pos, miss_neg); returns the chosen row, the scores in out_score
int thc_select(const double* scales, const int64_t* rows, int n, double* out_score) {
  std::vector<CvRow> t((size_t)n);
  for (int k = 0; k < n; ++k) {
    t[(size_t)k].scale = scales[k];
    t[(size_t)k].n_pos = rows[4 * k];
    t[(size_t)k].n_neg = rows[4 * k + 1];
    t[(size_t)k].miss_pos = rows[4 * k + 2];
    t[(size_t)k].miss_neg = rows[4 * k + 3];
  }
  const int best = cv_select(t);
  for (int k = 0; k < n; ++k) out_score[k] = t[(size_t)k].score;
  return best;
}

// The labels of one requested feature (frames only) against folds x scales; returns 1 with the message in msg
int thc_check_cv(const int* label_frames, int n, int folds, const double* scales, int n_scales, char* msg, int msg_cap) {
  TrainLabels L;
  L.requested[TF_PAW_BOTTOM] = true;
  for (int k = 0; k < n; ++k) L.points[TF_PAW_BOTTOM].push_back(TrainPoint{label_frames[k], 0, 0});
  TrainOptions o;
  o.cv_folds = folds;
  o.cv_scales.assign(scales, scales + n_scales);
  try {
    check_train_cv(L, o);
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)msg_cap, "%s", e.what());
    return 1;
  }
  return 0;
}

int64_t thc_objective(const uint8_t* X, int64_t pitch, const int8_t* y, const uint8_t* group, int64_t N, int D,
                      double c_pos, double c_neg, int held_out, const double* wb, double* z, double* a, double* F,
                      double* grad) {
  std::vector<double> t((size_t)N);
  return lmt_host_objective_heldout(X, pitch, y, group, N, D, c_pos, c_neg, held_out, wb, z, a, t.data(), F, grad);
}

int thc_linesearch(const int8_t* y, const uint8_t* group, const double* z, const double* xd, int64_t N, double c_pos,
                   double c_neg, int held_out, double wd, double dd, double gd, double* dF) {
  return lmt_host_linesearch_heldout(y, group, z, xd, N, c_pos, c_neg, held_out, wd, dd, gd, dF);
}

}  // extern "C"
