// TranscodeCli.cpp — the `LocoMouseTranscode` executable: any video LocoMouse
// reads, written again as an MJPEG AVI whose frames carry restart markers, so
// that the device decoder (LM_DECODE=device) takes its interval path on it:
// one lane per restart interval, no guess and no sync round.
// Not in the reference.
//
//   LocoMouseTranscode in.avi out.avi [quality[:restart_mcus]]
//
// The output is grey: channel 0 of every frame (all the detector ever reads),
// encoded on the device as a one-component JPEG (include/locomouse_encode.h,
// lm_enc_create_restart).  quality in 1..100 (92); restart_mcus in 0..65535
// (16; 0 writes no restart markers), in MCUs of 8 x 8 pixels.
//
// LM_DEVICE: the HIP device (0); LM_BATCH: frames per encoder call (64);
// LM_READ_THREADS: decode threads, as for LocoMouse.  Exit code 1 on any
// error; the argument and video checks come before any GPU call.
#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Media.hpp"
#include "VideoFrames.hpp"
#include "locomouse_encode.h"

namespace {

constexpr int kDefaultQuality = 92;
constexpr int kDefaultRestart = 16;  // MCUs ("interval path")

struct Encoder {
  lm_enc_ctx* c = nullptr;
  ~Encoder() { lm_enc_destroy(c); }
};

void check(lm_status s) {
  if (s != LM_OK) throw std::runtime_error(lm_last_error());
}

// A whole decimal number in lo..hi, or std::invalid_argument naming `what`.
int number(const std::string& text, const char* what, int lo, int hi, const std::string& spec) {
  size_t used = 0;
  int v = 0;
  try {
    v = std::stoi(text, &used);
  } catch (const std::exception&) {
    used = 0;
  }
  if (text.empty() || used != text.size() || text[0] == '+' || text[0] == ' ')
    throw std::invalid_argument("expected quality[:restart_mcus], not " + spec + ".");
  if (v < lo || v > hi)
    throw std::invalid_argument(std::string(what) + " must be in " + std::to_string(lo) + ".." + std::to_string(hi) + ", not " +
                                text + ".");
  return v;
}

int run(int argc, char** argv) {
  using namespace locomouse;
  if (argc < 3 || argc > 4) {
    std::cout << "Usage: LocoMouseTranscode in.avi out.avi [quality[:restart_mcus]]" << std::endl;
    return EXIT_FAILURE;
  }
  int quality = kDefaultQuality, restart = kDefaultRestart;
  if (argc == 4) {
    const std::string spec = argv[3];
    const size_t colon = spec.find(':');
    try {
      quality = number(spec.substr(0, colon), "quality", 1, 100, spec);
      if (colon != std::string::npos) restart = number(spec.substr(colon + 1), "restart_mcus", 0, 65535, spec);
    } catch (const std::invalid_argument& e) {
      std::cout << "Invalid inputs: " << e.what() << std::endl;
      return EXIT_FAILURE;
    }
  }
  const std::string in_file = argv[1], out_file = argv[2];
  int device = 0, batch = 64;
  if (const char* d = std::getenv("LM_DEVICE")) device = std::atoi(d);
  if (const char* b = std::getenv("LM_BATCH")) batch = std::max(1, std::min(LM_ENC_MAX_BATCH, std::atoi(b)));
  auto video = std::make_shared<AviReader>();
  if (!video->open(in_file)) {
    std::cout << "Invalid inputs: Could not open the video file: " << in_file << "." << std::endl;
    return EXIT_FAILURE;
  }
  const int rows = video->rows(), cols = video->cols();
  const int64_t slot = lm_enc_slot_bytes_restart(rows, cols, LM_ENC_GRAY8, restart);
  if (slot < 0) {
    std::cout << "Invalid inputs: the frames are too large for the encoder." << std::endl;
    return EXIT_FAILURE;
  }
  while (batch > 1 && slot * batch >= (int64_t)1 << 31) batch /= 2;  // (lm_enc_create's limit)
  int read_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  if (const char* t = std::getenv("LM_READ_THREADS")) read_threads = std::max(1, std::atoi(t));
  VideoFrames reader(video, read_threads);
  MjpegAviWriter avi;
  if (!avi.open(out_file, rows, cols, video->fps() > 0 ? video->fps() : 30)) {
    std::cout << "Invalid inputs: Could not open the output file: " << out_file << "." << std::endl;
    return EXIT_FAILURE;
  }
  // ---- from here on the device is used
  Encoder E;
  check(lm_enc_create_restart(device, rows, cols, LM_ENC_GRAY8, quality, batch, restart, &E.c));
  const size_t fb = (size_t)rows * (size_t)cols;
  std::vector<uint8_t> frames(fb * (size_t)batch);
  const uint32_t total = video->frame_count();
  uint64_t bytes = 0;
  for (uint32_t done = 0; done < total;) {
    const int want = (int)std::min<uint32_t>((uint32_t)batch, total - done);
    const int got = reader.read(frames.data(), want);
    if (got != want) throw std::runtime_error("Could not read frame " + std::to_string(done + (uint32_t)got) + " of the video.");
    lm_enc_result res{};
    check(lm_enc_encode(E.c, frames.data(), (int64_t)fb, got, &res));
    for (int i = 0; i < got; ++i) {
      if (!avi.add(res.data + res.offset[i], res.size[i]))
        throw std::runtime_error("Could not write frame " + std::to_string(done + (uint32_t)i) + " to " + out_file +
                                 " (a write error, or the file would pass 4 GiB).");
      bytes += res.size[i];
    }
    done += (uint32_t)got;
  }
  if (!avi.close()) throw std::runtime_error("Could not finish the output file: " + out_file + ".");
  std::cout << "Transcoded " << total << " frames of " << rows << " x " << cols << " to grey JPEG at quality " << quality
            << ", restart interval " << restart << " MCUs (" << bytes << " bytes): " << out_file << std::endl;
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
