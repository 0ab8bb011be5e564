// BackgroundCli.cpp — the `LocoMouseBackground` executable: the background.png
// the LocoMouse program takes, estimated from the video as its per-pixel
// temporal median (Background.hpp).  Not in the reference, whose background
// image comes from its MATLAB front end.
//
//   LocoMouseBackground video.avi out.png [stride [permille]]
//
// LM_DEVICE: the HIP device (0); LM_READ_THREADS: decode threads, as for
// LocoMouse.  Exit code 1 on any error; the argument and video checks come
// before any GPU call.
#include <cstdlib>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Background.hpp"
#include "Media.hpp"
#include "VideoFrames.hpp"

namespace {

int run(int argc, char** argv) {
  using namespace locomouse;
  if (argc < 3 || argc > 5) {
    std::cout << "Usage: LocoMouseBackground video.avi out.png [stride [permille]]" << std::endl;
    return EXIT_FAILURE;
  }
  BackgroundOptions opt;
  std::string spec = "median";
  for (int k = 3; k < argc; ++k) spec += std::string(":") + argv[k];
  try {
    parse_background_spec(spec, opt);
  } catch (const std::invalid_argument&) {
    std::cout << "Usage: LocoMouseBackground video.avi out.png [stride [permille]]  (stride >= 1, permille in 0..1000)"
              << std::endl;
    return EXIT_FAILURE;
  }
  const std::string video_file = argv[1], out_file = argv[2];
  auto video = std::make_shared<AviReader>();
  if (!video->open(video_file)) {
    std::cout << "Could not open the video file: " << video_file << "." << std::endl;
    return EXIT_FAILURE;
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
  std::vector<uint8_t> bkg;
  estimate_background(li, opt, bkg);
  if (!write_png_gray(out_file, video->rows(), video->cols(), bkg.data()))
    throw std::runtime_error("Could not write the background image: " + out_file + ".");
  std::cout << "Background of " << li.n_frames << " frames (stride " << opt.stride << ", permille " << opt.permille
            << ") written to " << out_file << std::endl;
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
