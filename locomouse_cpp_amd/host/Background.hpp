// Background.hpp — the background image estimated from the video itself
// (include/locomouse_bkg.h): the per-pixel temporal median, or another rank,
// of its channel-0 frames.  The reference only ever loads background.png
// (loadBackground, LocoMouse_class.cpp:405-419; subtract(F, BKG, F)); the
// image comes from the MATLAB front end its Readme points to.  Not in the
// reference.
#ifndef LOCOMOUSE_HOST_BACKGROUND_HPP
#define LOCOMOUSE_HOST_BACKGROUND_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "LocoMouse.hpp"

namespace locomouse {

struct BackgroundOptions {
  int stride = 1;      // every stride-th frame is sampled, from frame 0
  int permille = 500;  // rank = (permille * (K - 1)) / 1000 of each pixel's K sorted samples; 500: lower median
  int device = 0;      // HIP device
  int batch = 256;     // frames read at a time (one lm_bkg_push each)
};

// Reads in.n_frames frames of in.setup.video_rows x video_cols through
// in.read_frames (or in.read_frame when only that is given), decoded on the
// host, pushes every stride-th from page-locked memory, writes the image
// (rows * cols bytes) to `out` and calls in.rewind.  Throws
// std::runtime_error (with lm_last_error() for a failing lm_bkg_* call); a
// video whose sampled frames exceed LM_BKG_MAX_SAMPLES is refused before
// anything is read, with the smallest stride that fits in the message.
void estimate_background(const LocoMouse_Inputs& in, const BackgroundOptions& opt, std::vector<uint8_t>& out);

// "median[:stride[:permille]]" (the LM_BACKGROUND knob) into opt.stride /
// opt.permille; throws std::invalid_argument("LM_BACKGROUND: ...") for
// anything else.
void parse_background_spec(const std::string& spec, BackgroundOptions& opt);

}  // namespace locomouse

#endif
