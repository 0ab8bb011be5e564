// Calibration.hpp — the calibration.yml (ind_warp_mapping, view_boxes)
// estimated from a marker video (include/locomouse_calib.h): a pen tip moved
// through the corridor is found in both views of every frame on the device,
// and a polynomial column warp of the side view is fitted on the host so that
// the same physical point has the same x in both views.  The reference only
// ever loads the file (loadCalibration, LocoMouse_class.cpp:419-463;
// correctImage, :1337-1406); it comes from the MATLAB front end its Readme
// points to.  Not in the reference.
#ifndef LOCOMOUSE_HOST_CALIBRATION_HPP
#define LOCOMOUSE_HOST_CALIBRATION_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "LocoMouse.hpp"
#include "locomouse_calib.h"

namespace locomouse {

struct CalibrationOptions {
  lm_calib_opts detect{40, 12, 80, 12, 8, 0};  // threshold, radius, min_peak, min_area, max_stray
  int split_row = 0;                           // the side view is rows [0, split_row)
  int degree = 2;                              // of the column warp, 1..3
  double max_resid = 1.5;                      // samples further than this from the first fit are dropped, pixels
  std::vector<uint8_t> background;             // rows * cols bytes; empty: the video's median (estimate_background)
  int device = 0;                              // HIP device
  int batch = 256;                             // frames read at a time (one lm_calib_push each)
};

struct CalibrationResult {
  int rows = 0, cols = 0, split_row = 0;
  lm_calib_fit_result fit{};
  std::vector<int32_t> map;         // ind_warp_mapping, rows x cols
  int32_t view_boxes[8] = {0};      // side then bottom: x, y, width, height
  std::vector<double> samples;      // n_samples x 3: frame, xb, xs
  double background_ms = 0, detect_ms = 0, fit_ms = 0;  // wall time of the three stages
};

// A whole, non-negative decimal number of at most 9 digits, or -1 (the fields of LM_CALIB, the program's arguments).
long whole_number(const std::string& s);

// "threshold:radius:min_peak:min_area:max_stray:max_resid" (the LM_CALIB
// knob): fields from the left, whole numbers except the last, trailing fields
// optional.  Throws std::invalid_argument("LM_CALIB: ...") for anything else.
void parse_calibration_spec(const std::string& spec, CalibrationOptions& opt);

// Reads in.n_frames frames of in.setup.video_rows x video_cols through
// in.read_frames (or in.read_frame), pushes them from page-locked memory,
// fits and builds the map, and calls in.rewind.  Throws std::runtime_error:
// the argument checks come before any GPU call, and a refused fit carries the
// count or the range in its text.
void estimate_calibration(const LocoMouse_Inputs& in, const CalibrationOptions& opt, CalibrationResult& out);

// The file the program reads: ind_warp_mapping and view_boxes (dt: i), and,
// ignored by the reference, warp_coefficients (dt: d; the polynomial in
// t = (x - cols/2) / (cols/2), constant first), warp_range (lo, hi),
// warp_residuals (rms, largest), warp_counts (frames, samples, used) and
// warp_samples (frame, xb, xs per row).
void write_calibration_yaml(const std::string& path, const CalibrationResult& result);

}  // namespace locomouse

#endif
