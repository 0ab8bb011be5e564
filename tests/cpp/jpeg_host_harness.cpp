// jpeg_host_harness.cpp — the host mirror (LocoMouse) fed an MJPEG video from
// memory, with LocoMouse_Inputs::decode = host or device: the whole-video
// bounding-box pass (use_provided_bounding_box = 0) and the per-frame loop.
// Returns the per-frame corners, the box sizes and the candidate counts, so a
// test can require the two decode choices to give the same run.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "Jpeg.hpp"
#include "LocoMouse.hpp"

using namespace locomouse;

// 0 ok, 1 invalid_argument, 2 runtime_error (message in err).
extern "C" __attribute__((visibility("default"))) int jhh_run(
    const lm_setup* setup, const lm_params* params, const lm_model* model, const lm_bb_params* bb_params,
    const uint8_t* const* jpeg, const size_t* size, int n_frames, int batch, int device_decode, uint32_t* corners,
    lm_rect* sizes, int32_t* n_candidates, int32_t* fallbacks, char* err, int errlen) {
  try {
    LocoMouse_Inputs in;
    in.setup = *setup;
    in.params = *params;
    in.model = *model;
    in.n_frames = (uint32_t)n_frames;
    in.batch = batch;
    in.bb_params = *bb_params;
    const int rows = setup->video_rows, cols = setup->video_cols;
    const size_t fb = (size_t)rows * cols;
    int next = 0;
    in.read_frame = [&](uint8_t* dst) {
      return next < n_frames && decode_jpeg_channel0_into(jpeg[next], size[next], rows, cols, dst) && ++next;
    };
    in.read_frames = [&](uint8_t* dst, int n) {
      int k = 0;
      for (; k < n && next < n_frames; ++k, ++next)
        if (!decode_jpeg_channel0_into(jpeg[next], size[next], rows, cols, dst + (size_t)k * fb)) break;
      return k;
    };
    in.rewind = [&] { next = 0; };
    if (device_decode) {
      in.decode = LocoMouse_Inputs::Decode::device;
      in.read_compressed = [&](std::vector<std::vector<uint8_t>>& out, int n) {
        int k = 0;
        for (; k < n && next < n_frames; ++k, ++next) out.emplace_back(jpeg[next], jpeg[next] + size[next]);
        return k;
      };
    }
    std::unique_ptr<LocoMouse> L = LocoMouse_Initialize(in);
    L->getBoundingBox();
    L->initializeFeatureLoop();
    for (unsigned i = 0; i < L->N_frames(); ++i) {
      corners[3 * i] = L->bb_x_pos()[i];
      corners[3 * i + 1] = L->bb_y_bottom_pos()[i];
      corners[3 * i + 2] = L->bb_y_side_pos()[i];
    }
    sizes[0] = L->bb_side_mouse();
    sizes[1] = L->bb_bottom_mouse();
    for (unsigned i = 0; i < L->N_frames(); ++i) {
      L->readFrame();
      L->storePreviousImage();
    }
    const auto& bp = L->candidates_bottom_paw();
    const auto& sp = L->candidates_side_paw();
    for (unsigned i = 0; i < L->N_frames(); ++i) {
      n_candidates[2 * i] = (int32_t)bp[i].size();
      n_candidates[2 * i + 1] = (int32_t)sp[i].size();
    }
    *fallbacks = L->stage_times().decode_fallback_frames;
    return 0;
  } catch (const std::invalid_argument& e) {
    std::strncpy(err, e.what(), (size_t)errlen - 1);
    return 1;
  } catch (const std::exception& e) {
    std::strncpy(err, e.what(), (size_t)errlen - 1);
    return 2;
  }
}
