// bkg_host_harness.cpp — host/Background.hpp's checks that come before any GPU
// call, for tests/test_bkg.py: estimate_background's refusals and the
// LM_BACKGROUND parser.  Links liblocomouse_host.so.
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "Background.hpp"

extern "C" {

// estimate_background on a video of n_frames frames whose reader must never be
// called; returns 0 with the exception's text in msg, 1 when nothing was
// thrown, 2 when a frame was asked for.
int bhh_refusal(unsigned n_frames, int rows, int cols, int stride, int permille, char* msg, int cap) {
  locomouse::LocoMouse_Inputs in;
  in.n_frames = n_frames;
  in.setup.video_rows = rows;
  in.setup.video_cols = cols;
  bool read = false;
  in.read_frames = [&](uint8_t*, int) {
    read = true;
    return 0;
  };
  locomouse::BackgroundOptions opt;
  opt.stride = stride;
  opt.permille = permille;
  std::vector<uint8_t> out;
  try {
    locomouse::estimate_background(in, opt, out);
  } catch (const std::exception& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return read ? 2 : 0;
  }
  return 1;
}

// parse_background_spec: 0 and (stride, permille), or 1 and the message.
int bhh_parse(const char* spec, int* stride, int* permille, char* msg, int cap) {
  locomouse::BackgroundOptions opt;
  try {
    locomouse::parse_background_spec(spec, opt);
  } catch (const std::invalid_argument& e) {
    std::snprintf(msg, (size_t)cap, "%s", e.what());
    return 1;
  }
  *stride = opt.stride;
  *permille = opt.permille;
  return 0;
}
}
