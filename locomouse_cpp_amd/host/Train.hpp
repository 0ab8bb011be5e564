// Train.hpp — detector weights trained from labelled frames
// (include/locomouse_train.h): the model.yml the reference only ever loads
// (LocoMouse_Model, LocoMouse_class.cpp:3095-3162; its detectors come from
// the MATLAB front end, which trains linear SVMs on labelled patches).  Not in
// the reference.
//
// Labels are points (frame, column, row) in the corrected image, the
// zero-based coordinates of the exported tracks, so a corrected
// output_<stem>.yml is a label file.  Per requested feature:
//   positives   the labelled points;
//   negatives   neg_per_frame points per labelled frame from a splitmix64
//               sequence keyed by (feature, frame, index), inside the
//               feature's view box and at Chebyshev distance >= r_neg from
//               every label of that feature in that frame;
//   mining      up to `rounds` times: solve, put the detector into the model,
//               run the labelled frames through the detection path (the
//               LocoMouse mirror), add every candidate of the feature's list
//               that is >= r_neg from all its labels as a negative
//               (deduplicated by (frame, x, y)), and solve again; a round that
//               adds none ends it.  The tail detectors have no candidate list:
//               they are solved once.
//   costs       with cv_folds > 0, after the last mining round: the costs are
//               scaled by each of cv_scales in turn and scored by k-fold
//               cross-validation over the feature's labelled frames (frame
//               rank r of the sorted frames is fold r mod cv_folds, and every
//               sample of a frame, label, initial or mined negative, takes its
//               frame's fold), all folds x scales problems in one
//               lm_train_solve_many call; the scale with the smallest balanced
//               error of the held-out samples wins, and the detector is
//               lm_train_solve on all samples with the costs times that scale.
//               The mining rounds before it ran with the spec's own costs and
//               are not repeated.
#ifndef LOCOMOUSE_HOST_TRAIN_HPP
#define LOCOMOUSE_HOST_TRAIN_HPP

#include <cstdint>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "Inputs.hpp"
#include "LocoMouse.hpp"
#include "locomouse_train.h"

namespace locomouse {

enum TrainFeature { TF_PAW_BOTTOM = 0, TF_SNOUT_BOTTOM, TF_TAIL_BOTTOM, TF_PAW_SIDE, TF_SNOUT_SIDE, TF_TAIL_SIDE, TF_COUNT };
extern const char* const kTrainFeatureNames[TF_COUNT];  // "paw_bottom" ..
int train_feature_from_name(const std::string& name);   // -1: no such feature

struct TrainPoint {
  int frame, x, y;  // video frame; column, row in the corrected image
};
using TrainSeen = std::set<std::tuple<int, int, int>>;

struct TrainOptions {
  double c_pos = 10.0, c_neg = 1.0, eps = 1e-6;
  int rounds = 2, neg_per_frame = 60;
  int r_neg = 0;       // 0: max(kh, kw) / 4
  int max_iter = 200;  // outer iterations of a solve
  int cv_folds = 0;    // 0: no cross-validation; else 2..16
  std::vector<double> cv_scales;  // 1..16 distinct positive scales of (c_pos, c_neg); cv_folds x scales <= LM_TRAIN_MAX_PROBLEMS
};

// "c_pos:c_neg:eps:rounds:neg_per_frame" (the LM_TRAIN knob; trailing fields
// may be left out); throws std::invalid_argument("LM_TRAIN: ...").
void parse_train_spec(const std::string& spec, TrainOptions& opt);

// "folds:s1,s2,..." (the LM_TRAIN_CV knob): folds in 2..16, 1..16 scales, each
// positive and finite and at most once, folds x scales <= LM_TRAIN_MAX_PROBLEMS;
// throws std::invalid_argument("LM_TRAIN_CV: ...").
void parse_train_cv_spec(const std::string& spec, TrainOptions& opt);

struct TrainLabels {
  bool requested[TF_COUNT] = {false, false, false, false, false, false};
  std::vector<TrainPoint> points[TF_COUNT];
};

// A cost scale's held-out counts pooled over the folds (every sample is held out exactly once).
struct CvRow {
  double scale = 0;
  int64_t n_pos = 0, n_neg = 0, miss_pos = 0, miss_neg = 0;
  double score = 0;  // the balanced error 1/2 (miss_pos / n_pos + miss_neg / n_neg); a class without samples leaves its term out
};

struct TrainReport {
  struct Feature {
    int feature = -1, n_pos = 0, n_neg_initial = 0;
    std::vector<int> mined;  // negatives added per mining round
    lm_train_stats stats{};  // of the last solve
    std::vector<CvRow> cv;   // with cv_folds > 0: one row per scale, in cv_scales' order
    double cv_scale = 0;     // the chosen scale
  };
  std::vector<Feature> features;
  double gather_s = 0, solve_s = 0, mining_s = 0, cv_s = 0;
};

// The fold of every sample: sample_frames[i] is sample i's video frame; the
// distinct frames are sorted and frame rank r is fold r mod folds.  Pure host code.
std::vector<int32_t> cv_fold_of_samples(const std::vector<int>& sample_frames, int folds);

// Fills every row's score and returns the index of the row with the smallest;
// a tie goes to the smaller scale, which regularises more.  Scores are
// compared exactly, as the fractions of integers they are.  Pure host code.
int cv_select(std::vector<CvRow>& rows);

// The mined negatives of one round: the candidates, in their order, that are at
// Chebyshev distance >= r_neg from every label of their frame and whose
// (frame, x, y) is not in `seen`, which grows by what is taken.  Pure host code.
std::vector<TrainPoint> select_mined(const std::vector<TrainPoint>& candidates, const std::vector<TrainPoint>& labels,
                                     int r_neg, TrainSeen& seen);

// The initial negatives of one labelled frame (see above); `view` is clipped
// to the rows x cols image.  Fewer than neg_per_frame when the box has no room.
std::vector<TrainPoint> initial_negatives(int feature, int frame, const std::vector<TrainPoint>& labels, lm_rect view,
                                          int rows, int cols, int r_neg, int neg_per_frame);

// Checks the labels against the inputs (a frame past the video, a point
// outside the corrected image, a requested feature without labels): throws
// std::invalid_argument.  No device call.
void check_train_labels(const LocoMouse_Inputs& in, const TrainLabels& labels);

// With opt.cv_folds > 0: every requested feature has at least cv_folds labelled
// frames, and the folds and scales are in range; throws std::invalid_argument.
void check_train_cv(const TrainLabels& labels, const TrainOptions& opt);

// Trains every requested feature in turn, each on top of the detectors
// trained before it; out starts as a copy of base.  Reads the labelled frames
// through in.read_frames / in.read_frame (sequentially from frame 0) and
// calls in.rewind.  Throws std::invalid_argument for bad labels (before any
// device call) and std::runtime_error for a failing lm_* call.
void train_detectors(const LocoMouse_Inputs& in, const TrainLabels& labels, const TrainOptions& opt, const Model& base,
                     Model& out, TrainReport* report = nullptr);

}  // namespace locomouse

#endif
