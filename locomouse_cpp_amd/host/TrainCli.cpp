// TrainCli.cpp — the `LocoMouseTrain` executable: the model.yml the LocoMouse
// program takes, with detectors trained from labelled frames (Train.hpp).  Not
// in the reference, whose models come from its MATLAB front end.
//
//   LocoMouseTrain config.yml video.avi background.png calibration.yml L|R labels.yml model_in.yml model_out.yml
//                  [feature ...]
//
// labels.yml is FileStorage YAML: per feature, labels_<feature> is an integer
// n x 3 matrix of (frame, column, row) in the coordinates of
// output_<stem>.yml; the features are paw_bottom, snout_bottom, tail_bottom,
// paw_side, snout_side, tail_side (the four paws are one class).  Without
// feature arguments every feature labels.yml has is trained.  model_in.yml
// gives the detector sizes and the detectors that are not retrained;
// model_out.yml is written under the same twelve keys.
//
// LM_TRAIN=c_pos:c_neg:eps:rounds:neg_per_frame (10:1:1e-6:2:60); LM_METHOD:
// the LocoMouse method whose frame normalisation is used (0); LM_DEVICE,
// LM_BATCH, LM_BACKGROUND, LM_READ_THREADS as for LocoMouse; LM_TIMING prints
// the gather, solve, mining and cross-validation times.  LM_TRAIN_CV=folds:s1,s2,...
// (off): the costs are scaled by each s in turn, scored by cross-validation
// over the labelled frames in `folds` folds, and the best scale trains the
// detector (Train.hpp); a line per feature prints the table.  Malformed input is an
// "Invalid inputs: ..." error before a device is touched.  Exit code 1 on any
// error.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Background.hpp"
#include "FileStorage.hpp"
#include "Inputs.hpp"
#include "Media.hpp"
#include "Train.hpp"
#include "VideoFrames.hpp"

namespace locomouse {
namespace {

const char* kUsage =
    "Usage: LocoMouseTrain config.yml video.avi background.png calibration.yml L|R labels.yml model_in.yml "
    "model_out.yml [feature ...]";

void load_labels(const std::string& file, const std::vector<std::string>& wanted, TrainLabels& labels) {
  FsNode root;
  if (!read_file_storage(file, root)) throw std::invalid_argument("Could not open the labels file: " + file + ".");
  for (const std::string& name : wanted) {
    const int f = train_feature_from_name(name);
    if (f < 0) throw std::invalid_argument("Unknown feature: " + name + ".");
    labels.requested[f] = true;
  }
  for (int f = 0; f < TF_COUNT; ++f) {
    const std::string key = std::string("labels_") + kTrainFeatureNames[f];
    const FsNode& node = root[key];
    if (wanted.empty() && !node.empty()) labels.requested[f] = true;
    if (!labels.requested[f]) continue;
    const FsMat M = node.to_mat();
    if (M.empty()) throw std::invalid_argument(key + " is empty or undefined.");
    if (M.cols != 3) throw std::invalid_argument(key + " must be an n x 3 matrix (frame, column, row).");
    if (M.dt != 'i') throw std::invalid_argument(key + " must be an integer (dt: i) matrix.");
    for (int r = 0; r < M.rows; ++r)
      labels.points[f].push_back(TrainPoint{(int)M.at(r, 0), (int)M.at(r, 1), (int)M.at(r, 2)});
  }
}

int run(int argc, char** argv) {
  if (argc < 9) throw std::invalid_argument(kUsage);
  const std::string config_file = argv[1], video_file = argv[2], bkg_file = argv[3], calibration_file = argv[4],
                    flip_char = argv[5], labels_file = argv[6], model_in = argv[7], model_out = argv[8];
  std::vector<std::string> wanted(argv + 9, argv + argc);
  LocoMouse_Inputs li;
  DebugConfig dbg;
  std::string ref_path = argv[0];
  ref_path = ref_path.find_last_of('/') == std::string::npos ? "./" : ref_path.substr(0, ref_path.find_last_of('/') + 1);
  load_config(config_file, ref_path, li.params, li.bb_params, dbg);
  auto video = std::make_shared<AviReader>();
  if (!video->open(video_file)) throw std::invalid_argument("Could not open the video file: " + video_file + ".");
  li.n_frames = video->frame_count();
  if (li.n_frames < 1) throw std::invalid_argument("Error: Video has no images to read from.");
  BackgroundOptions bkg_opt;
  const char* bkg_spec = std::getenv("LM_BACKGROUND");
  if (bkg_spec) parse_background_spec(bkg_spec, bkg_opt);
  int br = 0, bc = 0;
  std::vector<uint8_t> bkg;
  if (!bkg_spec && !read_png_gray(bkg_file, br, bc, bkg))
    throw std::invalid_argument("Could not open the background image: " + bkg_file + ".");
  if (!bkg_spec && (bc != video->cols() || br != video->rows())) {
    std::ostringstream m;
    m << "Error: Background image does not match video size. Background image has size [" << bc << " x " << br
      << "] while Video has size [" << video->cols() << " x " << video->rows() << "].";
    throw std::invalid_argument(m.str());
  }
  Calibration cal;
  load_calibration(calibration_file, cal);
  if (flip_char != "L" && flip_char != "R") throw std::invalid_argument("Mouse side option must be either \"L\" or \"R\".");
  Model base;
  load_model(model_in, base);
  TrainLabels labels;
  load_labels(labels_file, wanted, labels);
  TrainOptions opt;
  if (const char* spec = std::getenv("LM_TRAIN")) parse_train_spec(spec, opt);
  if (const char* spec = std::getenv("LM_TRAIN_CV")) parse_train_cv_spec(spec, opt);
  int method = 0;
  if (const char* m = std::getenv("LM_METHOD")) {
    method = std::atoi(m);
    if (method < 0 || method > 2) throw std::invalid_argument("LM_METHOD must be 0, 1 or 2.");
  }
  if (li.params.transform_gray_values && !li.params.use_reference_image_brightness)
    throw std::invalid_argument("transform_gray_values: that table moves with the per-frame crop; patches are not "
                                "gathered through it.");
  li.setup.method = method;
  li.setup.flip = flip_char == "L";
  li.setup.video_rows = video->rows();
  li.setup.video_cols = video->cols();
  li.setup.background = bkg.data();
  li.setup.calib_rows = cal.rows;
  li.setup.calib_cols = cal.cols;
  li.setup.ind_warp_mapping = cal.map.data();
  li.setup.view_box_side = cal.side_view;
  li.setup.view_box_bottom = cal.bottom_view;
  li.model = base.m;
  check_train_labels(li, labels);
  check_train_cv(labels, opt);
  {  // the output must be writable before the work is done
    std::FILE* f = std::fopen(model_out.c_str(), "a");
    if (!f) throw std::invalid_argument("Could not create the model file: " + model_out + ".");
    std::fclose(f);
  }
  int read_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  if (const char* t = std::getenv("LM_READ_THREADS")) read_threads = std::max(1, std::atoi(t));
  auto reader = std::make_shared<VideoFrames>(video, read_threads);
  li.read_frame = [reader](uint8_t* dst) { return reader->read(dst); };
  li.read_frames = [reader](uint8_t* dst, int n) { return reader->read(dst, n); };
  li.rewind = [reader] { reader->rewind(); };
  if (const char* d = std::getenv("LM_DEVICE")) li.device = std::atoi(d);
  if (const char* b = std::getenv("LM_BATCH")) li.batch = std::max(1, std::atoi(b));
  // ---- from here on the device is used
  if (bkg_spec) {
    bkg_opt.device = li.device;
    bkg_opt.batch = li.batch;
    estimate_background(li, bkg_opt, bkg);
    li.setup.background = bkg.data();
  }
  Model out;
  TrainReport rep;
  train_detectors(li, labels, opt, base, out, &rep);
  write_model(model_out, out.m);
  for (const TrainReport::Feature& f : rep.features) {
    std::cout << kTrainFeatureNames[f.feature] << ": " << f.n_pos << " positives, " << f.n_neg_initial
              << " initial negatives, mined";
    for (int m : f.mined) std::cout << " " << m;
    if (f.mined.empty()) std::cout << " none";
    std::cout << "; objective " << f.stats.objective << ", gradient " << f.stats.grad_norm << " of "
              << f.stats.grad_norm0 << ", " << f.stats.outer_iters << " outer and " << f.stats.cg_iters
              << " CG iterations, " << (f.stats.converged ? "converged" : "NOT converged") << std::endl;
    if (!f.cv.empty()) {
      std::cout << kTrainFeatureNames[f.feature] << " cv: " << opt.cv_folds << " folds;";
      for (const CvRow& r : f.cv)
        std::cout << " scale " << r.scale << ": missed " << r.miss_pos << "/" << r.n_pos << " positives, " << r.miss_neg
                  << "/" << r.n_neg << " negatives, score " << r.score << ";";
      std::cout << " chosen scale " << f.cv_scale << std::endl;
    }
  }
  std::cout << "Model written to " << model_out << std::endl;
  if (std::getenv("LM_TIMING"))
    std::cout << "LM_TIMING gather_ms " << 1e3 * rep.gather_s << " solve_ms " << 1e3 * rep.solve_s << " mining_ms "
              << 1e3 * rep.mining_s << " cv_ms " << 1e3 * rep.cv_s << std::endl;
  return EXIT_SUCCESS;
}

}  // namespace
}  // namespace locomouse

int main(int argc, char* argv[]) {
  try {
    return locomouse::run(argc, argv);
  } catch (const std::invalid_argument& e) {
    std::cout << "Invalid inputs: " << e.what() << std::endl;
  } catch (const std::exception& e) {
    std::cout << "Runtime Error: " << e.what() << std::endl;
  }
  return EXIT_FAILURE;
}
