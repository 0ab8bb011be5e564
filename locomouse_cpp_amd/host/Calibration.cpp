// Calibration.cpp — see Calibration.hpp.
#include "Calibration.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "../csrc/lm_calib_core.h"
#include "Background.hpp"
#include "FileStorage.hpp"
#include "locomouse_bkg.h"

namespace locomouse {

namespace {

struct Pinned {  // lm_host_alloc
  uint8_t* p = nullptr;
  ~Pinned() { lm_host_free(p); }
};

struct Detector {
  lm_calib_ctx* c = nullptr;
  ~Detector() { lm_calib_destroy(c); }
};

void check(lm_status s) {
  if (s != LM_OK) throw std::runtime_error(std::string("estimate_calibration: ") + lm_last_error());
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

long whole_number(const std::string& s) {
  if (s.empty() || s.size() > 9) return -1;
  long v = 0;
  for (char ch : s) {
    if (ch < '0' || ch > '9') return -1;
    v = v * 10 + (ch - '0');
  }
  return v;
}

void parse_calibration_spec(const std::string& spec, CalibrationOptions& opt) {
  std::vector<std::string> part(1);
  for (char ch : spec) {
    if (ch == ':')
      part.emplace_back();
    else
      part.back().push_back(ch);
  }
  if (part.size() > 6)
    throw std::invalid_argument("LM_CALIB: expected threshold:radius:min_peak:min_area:max_stray:max_resid, not " + spec + ".");
  static const char* const names[5] = {"threshold", "radius", "min_peak", "min_area", "max_stray"};
  int32_t* const field[5] = {&opt.detect.threshold, &opt.detect.radius, &opt.detect.min_peak, &opt.detect.min_area,
                             &opt.detect.max_stray};
  for (size_t k = 0; k < part.size() && k < 5; ++k) {
    const long v = whole_number(part[k]);
    if (v < 0) throw std::invalid_argument(std::string("LM_CALIB: ") + names[k] + " must be a whole number, not " + part[k] + ".");
    *field[k] = (int32_t)v;
  }
  if (part.size() == 6) {
    char* end = nullptr;
    const double v = part[5].empty() ? 0.0 : std::strtod(part[5].c_str(), &end);
    if (part[5].empty() || *end != '\0' || !std::isfinite(v) || !(v > 0.0))
      throw std::invalid_argument("LM_CALIB: max_resid must be a positive number, not " + part[5] + ".");
    opt.max_resid = v;
  }
  if (const char* why = lmc_check_opts(opt.detect)) throw std::invalid_argument(std::string("LM_CALIB: ") + why + ".");
}

void estimate_calibration(const LocoMouse_Inputs& in, const CalibrationOptions& opt, CalibrationResult& out) {
  const int rows = in.setup.video_rows, cols = in.setup.video_cols;
  if (rows <= 0 || cols <= 0) throw std::runtime_error("estimate_calibration: the video has no size");
  if (const char* why = lmc_check_shape(rows, cols, opt.split_row))
    throw std::runtime_error(std::string("estimate_calibration: ") + why + " (" + std::to_string(rows) + " x " +
                             std::to_string(cols) + ", split_row " + std::to_string(opt.split_row) + ")");
  if (const char* why = lmc_check_opts(opt.detect)) throw std::runtime_error(std::string("estimate_calibration: ") + why);
  if (opt.degree < 1 || opt.degree > LM_CALIB_MAX_DEGREE) throw std::runtime_error("estimate_calibration: degree must be 1, 2 or 3");
  if (!(opt.max_resid > 0.0)) throw std::runtime_error("estimate_calibration: max_resid must be positive");
  if (!in.read_frames && !in.read_frame) throw std::runtime_error("estimate_calibration: no frame reader");
  const int64_t total = in.n_frames;
  if (total < 1) throw std::runtime_error("estimate_calibration: the video has no frames");
  if (total > LM_CALIB_MAX_FRAMES)
    throw std::runtime_error("estimate_calibration: " + std::to_string(total) + " frames exceed the " +
                             std::to_string(LM_CALIB_MAX_FRAMES) + " one estimate takes.");
  const size_t fb = (size_t)rows * cols;
  if (!opt.background.empty() && opt.background.size() != fb)
    throw std::runtime_error("estimate_calibration: the background image is not " + std::to_string(rows) + " x " +
                             std::to_string(cols));

  auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> bkg = opt.background;
  if (bkg.empty()) {  // the video's median; every stride-th frame when the video has more than one estimate takes
    BackgroundOptions b;
    b.stride = (int)((total + LM_BKG_MAX_SAMPLES - 1) / LM_BKG_MAX_SAMPLES);
    b.permille = 500;
    b.device = opt.device;
    b.batch = opt.batch;
    estimate_background(in, b, bkg);
  }
  out.background_ms = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  const int batch = (int)std::min<int64_t>(std::max(opt.batch, 1), total);
  Detector D;
  check(lm_calib_create(opt.device, rows, cols, opt.split_row, batch, &opt.detect, &D.c));
  check(lm_calib_set_background(D.c, bkg.data()));
  Pinned buf;
  check(lm_host_alloc(fb * (size_t)batch, reinterpret_cast<void**>(&buf.p)));
  for (int64_t first = 0; first < total;) {
    const int want = (int)std::min<int64_t>(batch, total - first);
    int got = 0;
    if (in.read_frames) {
      got = in.read_frames(buf.p, want);
    } else {
      while (got < want && in.read_frame(buf.p + (size_t)got * fb)) ++got;
    }
    if (got != want)
      throw std::runtime_error("estimate_calibration: failed to read frame " + std::to_string(first + std::max(got, 0)) +
                               " of " + std::to_string(total));
    check(lm_calib_push(D.c, buf.p, (int64_t)fb, got));
    first += got;
  }
  std::vector<lm_calib_record> rec((size_t)total * 2);
  check(lm_calib_read(D.c, 0, (int32_t)total, rec.data()));
  if (in.rewind) in.rewind();
  out.detect_ms = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  out.rows = rows;
  out.cols = cols;
  out.split_row = opt.split_row;
  std::vector<LmcSample> sm;
  lmc_samples(rec.data(), (int)total, opt.detect, sm);
  out.samples.clear();
  for (const LmcSample& s : sm) {
    out.samples.push_back((double)s.frame);
    out.samples.push_back(s.xb);
    out.samples.push_back(s.xs);
  }
  check(lm_calib_fit(rec.data(), (int32_t)total, rows, cols, opt.split_row, &opt.detect, opt.degree, opt.max_resid, &out.fit));
  out.map.assign(fb, 0);
  check(lm_calib_map(&out.fit, rows, cols, opt.split_row, out.map.data(), out.view_boxes));
  out.fit_ms = ms_since(t0);
}

void write_calibration_yaml(const std::string& path, const CalibrationResult& r) {
  if (r.map.size() != (size_t)r.rows * (size_t)r.cols || r.map.empty())
    throw std::runtime_error("write_calibration_yaml: the result holds no map");
  FsWriter fs(path);
  if (!fs.isOpened()) throw std::runtime_error("Could not write the calibration file: " + path + ".");
  fs << "ind_warp_mapping";
  fs.write_mat_i(r.map.data(), r.rows, r.cols);
  fs << "view_boxes";
  fs.write_mat_i(r.view_boxes, 2, 4);
  fs << "warp_coefficients";
  fs.write_mat_d(r.fit.coef, 1, r.fit.degree + 1);
  const double range[2] = {r.fit.lo, r.fit.hi}, resid[2] = {r.fit.rms, r.fit.max_abs_resid};
  fs << "warp_range";
  fs.write_mat_d(range, 1, 2);
  fs << "warp_residuals";
  fs.write_mat_d(resid, 1, 2);
  const int counts[3] = {r.fit.n_frames, r.fit.n_samples, r.fit.n_used};
  fs << "warp_counts";
  fs.write_mat_i(counts, 1, 3);
  fs << "warp_samples";
  fs.write_mat_d(r.samples.data(), (int)(r.samples.size() / 3), 3);
  fs.release();
}

}  // namespace locomouse
