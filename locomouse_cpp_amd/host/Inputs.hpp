// Inputs.hpp — the files the programs take, read into the C-ABI's structs:
// config.yml (LocoMouse_Parameters, LocoMouse_class.cpp:4-249), the model file
// (LocoMouse_Model, :3095-3162) and the calibration file
// (LocoMouse_ParseInputs.cpp:62-99), with the reference's messages; and the
// model file written back under the reference's twelve keys (not in the
// reference, whose models come from its MATLAB front end).  Shared by the
// LocoMouse and LocoMouseTrain programs.
#ifndef LOCOMOUSE_HOST_INPUTS_HPP
#define LOCOMOUSE_HOST_INPUTS_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "locomouse_hip.h"

namespace locomouse {

struct DebugConfig {
  bool verbose = false;  // LM_DEBUG (verbose_debug, :17-19)
  int n_frames = 0;      // LM_N_FRAMES_TO_DEBUG (N_debug_frames, :21-26)
};

// config.yml's reference image (use_reference_image_brightness, :160-189), as
// read_png_gray hands it: a colour file is converted to grey, where the
// reference's imread would have handed computeNormalizedCDF channel 0.
struct ReferenceImage {
  int rows = 0, cols = 0;
  std::vector<uint8_t> px;  // rows x cols; empty: none was read
};

// Keys in the reference's order, its messages, OpenCV's missing-key-reads-0
// semantics.  Throws std::invalid_argument.  ref: where the reference image's
// pixels go when use_reference_image_brightness opened it (null: dropped).
void load_config(const std::string& file, const std::string& ref_path, lm_params& P, lm_bb_params& B, DebugConfig& D,
                 ReferenceImage* ref = nullptr);

// The six detectors in the file's order: paw_side, paw_bottom, tail_side,
// tail_bottom, snout_side, snout_bottom.  m's weight pointers point into w:
// call rebind() after copying a Model.
struct Model {
  std::vector<double> w[6];
  lm_model m{};
  lm_detector* detector(int k);  // k in the file's order
  void rebind();
};
extern const char* const kModelNames[6];  // modelPaw_side ..
extern const char* const kModelBiases[6];  // biasPaw_side ..

void load_model(const std::string& file, Model& M);
// FsWriter: each model<Feature>_<view> as a double matrix, each bias<Feature>_<view> as a real.
void write_model(const std::string& file, const lm_model& m);

struct Calibration {
  std::vector<int32_t> map;  // ind_warp_mapping, rows x cols
  int rows = 0, cols = 0;
  lm_rect side_view{}, bottom_view{};  // view_boxes
};
void load_calibration(const std::string& file, Calibration& C);

}  // namespace locomouse

#endif
