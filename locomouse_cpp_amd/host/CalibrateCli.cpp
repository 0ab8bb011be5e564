// CalibrateCli.cpp — the `LocoMouseCalibrate` executable: the calibration.yml
// the LocoMouse program takes, estimated from a video of a marker moved
// through the corridor and seen in both views (Calibration.hpp).  Not in the
// reference, whose calibration file comes from its MATLAB front end.
//
//   LocoMouseCalibrate video.avi out.yml split_row [degree]
//
// split_row: the first row of the bottom view; degree: of the column warp (1,
// 2 or 3; 2).  LM_CALIB=threshold:radius:min_peak:min_area:max_stray:max_resid
// (trailing fields optional); LM_CALIB_BACKGROUND=file.png: the background to
// subtract instead of the video's median; LM_DEVICE: the HIP device (0);
// LM_READ_THREADS: decode threads and LM_BATCH: frames per push, as for
// LocoMouse; LM_TIMING: print the wall time of the stages.  Exit code 1 on any
// error; the argument, video and image checks come before any GPU call.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Calibration.hpp"
#include "Media.hpp"
#include "VideoFrames.hpp"

namespace {

const char kUsage[] = "Usage: LocoMouseCalibrate video.avi out.yml split_row [degree]";

int run(int argc, char** argv) {
  using namespace locomouse;
  const long split = argc >= 4 ? locomouse::whole_number(argv[3]) : -1;
  const long degree = argc == 5 ? locomouse::whole_number(argv[4]) : 2;
  if (argc < 4 || argc > 5 || split < 1 || degree < 1 || degree > 3) {
    std::cout << kUsage << "  (split_row >= 1, degree 1, 2 or 3)" << std::endl;
    return EXIT_FAILURE;
  }
  CalibrationOptions opt;
  opt.split_row = (int)split;
  opt.degree = (int)degree;
  if (const char* spec = std::getenv("LM_CALIB")) parse_calibration_spec(spec, opt);
  const std::string video_file = argv[1], out_file = argv[2];
  auto video = std::make_shared<AviReader>();
  if (!video->open(video_file)) {
    std::cout << "Could not open the video file: " << video_file << "." << std::endl;
    return EXIT_FAILURE;
  }
  if (const char* file = std::getenv("LM_CALIB_BACKGROUND")) {
    int r = 0, c = 0;
    if (!read_png_gray(file, r, c, opt.background))
      throw std::runtime_error(std::string("Could not read the background image: ") + file + ".");
    if (r != video->rows() || c != video->cols())
      throw std::runtime_error(std::string("The background image ") + file + " is " + std::to_string(r) + " x " +
                               std::to_string(c) + ", the video " + std::to_string(video->rows()) + " x " +
                               std::to_string(video->cols()) + ".");
  }
  LocoMouse_Inputs li;
  li.n_frames = video->frame_count();
  li.setup.video_rows = video->rows();
  li.setup.video_cols = video->cols();
  int read_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  if (const char* t = std::getenv("LM_READ_THREADS")) read_threads = std::max(1, std::atoi(t));
  auto reader = std::make_shared<VideoFrames>(video, read_threads);
  li.read_frame = [reader](uint8_t* dst) { return reader->read(dst); };
  li.read_frames = [reader](uint8_t* dst, int n) { return reader->read(dst, n); };
  li.rewind = [reader] { reader->rewind(); };
  if (const char* d = std::getenv("LM_DEVICE")) opt.device = std::atoi(d);
  if (const char* b = std::getenv("LM_BATCH")) opt.batch = std::max(1, std::atoi(b));
  CalibrationResult res;
  estimate_calibration(li, opt, res);
  const auto t0 = std::chrono::steady_clock::now();
  write_calibration_yaml(out_file, res);
  const double write_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "Calibration of " << res.fit.n_frames << " frames: " << res.fit.n_used << " of " << res.fit.n_samples
            << " samples used, rms " << res.fit.rms << " px, largest residual " << res.fit.max_abs_resid
            << " px, columns " << res.fit.lo << " to " << res.fit.hi << ", written to " << out_file << std::endl;
  if (std::getenv("LM_TIMING"))
    std::cout << "LM_TIMING background_ms " << res.background_ms << " detect_ms " << res.detect_ms << " fit_ms "
              << res.fit_ms << " write_ms " << write_ms << " decode_threads " << reader->threads() << std::endl;
  return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char* argv[]) {
  try {
    return run(argc, argv);
  } catch (const std::exception& e) {
    std::cout << "Runtime Error: " << e.what() << std::endl;
    return EXIT_FAILURE;
  }
}
