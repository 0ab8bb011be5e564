// calib_host_harness.cpp — for tests/test_calib.py, without a GPU: the record
// of csrc/lm_calib_core.h on the host, and host/Calibration.hpp's LM_CALIB
// parser, the checks of estimate_calibration that precede any GPU call, and
// write_calibration_yaml.  Links liblocomouse_host.so.
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "Calibration.hpp"
#include "lm_calib_core.h"

extern "C" {

// lmc_host_record for n frames `pitch` bytes apart: out[n][2], side then bottom.
int chh_records(const uint8_t* frames, int64_t pitch, int n, const uint8_t* bkg, int rows, int cols, int split_row,
                const int32_t* opts, lm_calib_record* out) {
  lm_calib_opts o;
  std::memcpy(&o, opts, sizeof o);
  if (lmc_check_opts(o) || lmc_check_shape(rows, cols, split_row) || pitch < (int64_t)rows * cols) return 1;
  for (int f = 0; f < n; ++f)
    for (int view = 0; view < 2; ++view)
      lmc_host_record(frames + (int64_t)f * pitch, bkg, rows, cols, split_row, view, o, out + 2 * f + view);
  return 0;
}

// parse_calibration_spec: 0 and the fields, or 1 and the message.
int chh_parse(const char* spec, int32_t* five, double* max_resid, char* msg, int cap) {
  locomouse::CalibrationOptions opt;
  try {
    locomouse::parse_calibration_spec(spec, opt);
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return 1;
  }
  const int32_t v[5] = {opt.detect.threshold, opt.detect.radius, opt.detect.min_peak, opt.detect.min_area,
                        opt.detect.max_stray};
  std::memcpy(five, v, sizeof v);
  *max_resid = opt.max_resid;
  return 0;
}

// estimate_calibration on a video whose reader must never be called; returns 0
// with the exception's text in msg, 1 when nothing was thrown, 2 when a frame
// was asked for.
int chh_refusal(unsigned n_frames, int rows, int cols, int split_row, int degree, char* msg, int cap) {
  locomouse::LocoMouse_Inputs in;
  in.n_frames = n_frames;
  in.setup.video_rows = rows;
  in.setup.video_cols = cols;
  bool read = false;
  in.read_frames = [&](uint8_t*, int) {
    read = true;
    return 0;
  };
  locomouse::CalibrationOptions opt;
  opt.split_row = split_row;
  opt.degree = degree;
  locomouse::CalibrationResult out;
  try {
    locomouse::estimate_calibration(in, opt, out);
  } catch (const std::exception& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return read ? 2 : 0;
  }
  return 1;
}

// write_calibration_yaml of the given pieces: 0, or 1 and the message.
int chh_write_yaml(const char* path, int rows, int cols, int split_row, const lm_calib_fit_result* fit, const int32_t* map,
                   const int32_t* boxes, const double* samples, int n_samples, char* msg, int cap) {
  locomouse::CalibrationResult r;
  r.rows = rows;
  r.cols = cols;
  r.split_row = split_row;
  r.fit = *fit;
  r.map.assign(map, map + (size_t)rows * cols);
  std::memcpy(r.view_boxes, boxes, sizeof r.view_boxes);
  r.samples.assign(samples, samples + (size_t)n_samples * 3);
  try {
    locomouse::write_calibration_yaml(path, r);
  } catch (const std::exception& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return 1;
  }
  return 0;
}
}
