// Inputs.cpp — see Inputs.hpp.
#include "Inputs.hpp"

#include <cstring>
#include <iostream>
#include <stdexcept>

#include "FileStorage.hpp"
#include "Media.hpp"

namespace locomouse {

const char* const kModelNames[6] = {"modelPaw_side", "modelPaw_bottom", "modelTail_side",
                                    "modelTail_bottom", "modelSnout_side", "modelSnout_bottom"};
const char* const kModelBiases[6] = {"biasPaw_side", "biasPaw_bottom", "biasTail_side",
                                     "biasTail_bottom", "biasSnout_side", "biasSnout_bottom"};

lm_detector* Model::detector(int k) {
  lm_detector* dst[6] = {&m.paw_side, &m.paw_bottom, &m.tail_side, &m.tail_bottom, &m.snout_side, &m.snout_bottom};
  return dst[k];
}

void Model::rebind() {
  for (int k = 0; k < 6; ++k) detector(k)->weights = w[k].data();
}

// LocoMouse_Parameters (LocoMouse_class.cpp:4-249): keys in the reference's
// order, its messages, OpenCV's missing-key-reads-0 semantics.
void load_config(const std::string& file, const std::string& ref_path, lm_params& P, lm_bb_params& B,
                 DebugConfig& D, ReferenceImage* ref) {
  FsNode c;
  if (!read_file_storage(file, c)) throw std::invalid_argument("Failed to read config file: " + file + ".");
  const std::string E = "Invalid configuration parameter: ";
  auto bad = [&](const std::string& m) { throw std::invalid_argument(E + m); };
  auto num = [](double v) { return std::to_string(v); };
  D.verbose = c["verbose_debug"].to_int() != 0;
  D.n_frames = c["N_debug_frames"].to_int();
  if (D.n_frames < 0) bad("N_debug_frames must not be negative.");
  P.conn_comp_connectivity = c["conn_comp_connectivity"].to_int();
  if (P.conn_comp_connectivity != 4 && P.conn_comp_connectivity != 8)
    bad("conn_comp_connectivity must be either 4 or 8. Was " + std::to_string(P.conn_comp_connectivity) + ".");
  B.conn_comp_connectivity = P.conn_comp_connectivity;
  B.median_filter_size = c["median_filter_size"].to_int();
  if (B.median_filter_size % 2 == 0)
    bad("median_filter_size must be odd. Was " + std::to_string(B.median_filter_size) + ".");
  B.min_pixel_visible = c["min_pixel_visible"].to_int();
  if (B.min_pixel_visible < 0)
    bad("min_pixel_visible must be non-negative. Was " + std::to_string(B.min_pixel_visible) + ".");
  P.side_bottom_min_overlap = c["side_bottom_min_overlap"].to_double();
  if (P.side_bottom_min_overlap < 0 || P.side_bottom_min_overlap > 1)
    bad("side_bottom_min_overlap must belong to [0,1]. Was " + num(P.side_bottom_min_overlap) + ".");
  auto nonneg_int = [&](const char* key, int32_t& dst, const char* text) {
    dst = c[key].to_int();
    if (dst < 0) bad(std::string(key) + text + std::to_string(dst) + ".");
  };
  nonneg_int("max_displacement_bottom", P.max_displacement_bottom, " must be non-negative. Was ");
  nonneg_int("max_displacement_side", P.max_displacement_side, " must be non-negative. Was ");
  nonneg_int("occlusion_grid_spacing_pixels_side", P.occlusion_grid_spacing_pixels_side, " must be non-negative. Was ");
  nonneg_int("occlusion_grid_spacing_pixels_bottom", P.occlusion_grid_spacing_pixels_bottom,
             " must be non-negative.. Was ");
  P.occlusion_grid_max_width = c["occlusion_grid_max_width"].to_double();
  if (P.occlusion_grid_max_width < 0 || P.occlusion_grid_max_width > 1)
    bad("occlusion_grid_max_width must be non-negative. Was " + num(P.occlusion_grid_max_width) + ".");
  P.tail_sub_bounding_box = c["tail_sub_bounding_box"].to_double();
  if (P.tail_sub_bounding_box < 0 || P.tail_sub_bounding_box > 1)
    bad("tail_sub_bounding_box must be non-negative. Was " + num(P.tail_sub_bounding_box) + ".");
  auto nonneg = [&](const char* key, double& dst) {
    dst = c[key].to_double();
    if (dst < 0) bad(std::string(key) + " must be non-negative. Was " + num(dst) + ".");
  };
  nonneg("alpha_vel_bottom", P.alpha_vel_bottom);
  nonneg("alpha_vel_side", P.alpha_vel_side);
  nonneg("pairwise_occluded_cost", P.pairwise_occluded_cost);
  B.moving_average_window = c["moving_average_window"].to_int();
  if (B.moving_average_window % 2 == 0)
    bad("moving_average_window must be odd. Was " + std::to_string(B.moving_average_window) + ".");
  const FsMat W = c["location_prior"].to_mat();
  if (W.cols != 7 || W.rows != 5) bad("location_prior must be a 5x7 matrix. Was " + std::to_string(W.rows) + ".");
  if (W.dt != 'd') bad("location_prior must be a double (dt: d) matrix.");  // read through ptr<double>
  for (int r = 0; r < 5; ++r)
    P.location_prior[r] = lm_location_prior{W.at(r, 0), W.at(r, 1), W.at(r, 2), W.at(r, 3),
                                            W.at(r, 4), W.at(r, 5), W.at(r, 6)};
  P.transform_gray_values = c["transform_gray_values"].to_int();
  P.use_reference_image_brightness = c["use_reference_image_brightness"].to_int();
  bool both = false;
  if (P.transform_gray_values & P.use_reference_image_brightness) {
    std::cout << "Only one of 'use_reference_image_brightness' or 'transform_gray_values' should be true. Attempting "
                 "to read reference image..."
              << std::endl;
    both = true;
  }
  if (P.use_reference_image_brightness) {
    const std::string name = c["reference_image_path"].to_string();
    int r = 0, cc = 0;
    std::vector<uint8_t> px;
    if (!read_png_gray(name, r, cc, px) && !read_png_gray(ref_path + "/" + name, r, cc, px)) {
      if (both) {
        std::cout << "Could not open the reference image. Applying the provided transformation on the gray levels..."
                  << std::endl;
        P.use_reference_image_brightness = 0;
        both = false;
      } else {
        bad("Failed to open reference image: " + name + ".");
      }
    } else if (ref) {
      ref->rows = r;
      ref->cols = cc;
      ref->px = std::move(px);
    }
  }
  if (P.transform_gray_values & ~(int)both) {
    const FsMat G = c["gray_value_transformation"].to_mat();
    if (G.empty()) bad("Could not load the gray level transformation from the config file.");
    if (G.rows != 1 || G.cols != 256)
      bad("The gray level transformation must be a 1x256 matrix, was " + std::to_string(G.rows) + "x" +
          std::to_string(G.cols) + ".");
    for (int k = 0; k < 256; ++k) P.gray_value_transformation[k] = (float)G.v[k];
    // the table keeps its FileStorage depth: LUT() gives its output that type (:1448)
    static const char kDt[] = "ucwsifd";
    const char* d = std::strchr(kDt, G.dt);
    P.gray_value_transformation_depth = d ? (int32_t)(d - kDt) : LM_DEPTH_64F;
  }
  P.use_provided_bounding_box = c["use_provided_bounding_box"].to_int();
  if (P.use_provided_bounding_box) {
    const FsMat S = c["bounding_box_side"].to_mat();
    if (S.rows != 1 || S.cols != 4) {
      std::cout << S.rows << " " << S.cols << std::endl;
      bad("bounding_box_side must be a 1x4 OpenCV matrix.");
    }
    P.bounding_box_side = lm_rect{(int)S.v[0], (int)S.v[1], (int)S.v[2], (int)S.v[3]};
    const FsMat Bb = c["bounding_box_bottom"].to_mat();
    if (Bb.rows != 1 || Bb.cols != 4) bad("bounding_box_bottom must be a 1x4 OpenCV matrix.");
    if (Bb.dt != 'i')
      std::cout << "bounding_box_bottom must be provided as a 1x4 opencv matrix of type in (yml: i)." << std::endl;
    P.bounding_box_bottom = lm_rect{(int)Bb.v[0], (int)Bb.v[1], (int)Bb.v[2], (int)Bb.v[3]};
  }
}

void load_model(const std::string& file, Model& M) {
  FsNode c;
  if (!read_file_storage(file, c)) throw std::invalid_argument("Error: Could not open the model file: " + file + "\n");
  const char* const* names = kModelNames;
  const char* const* biases = kModelBiases;
  lm_detector* dst[6];
  for (int k = 0; k < 6; ++k) dst[k] = M.detector(k);
  for (int k = 0; k < 6; ++k) {
    const FsMat W = c[names[k]].to_mat();
    if (W.empty()) throw std::invalid_argument(std::string("Error: ") + names[k] + " cannot be empty." + file + "\n");
    M.w[k] = W.v;
    dst[k]->rows = W.rows;
    dst[k]->cols = W.cols;
  }
  for (int k = 0; k < 6; ++k) {
    dst[k]->weights = M.w[k].data();
    dst[k]->bias = c[biases[k]].to_double();
  }
}

void write_model(const std::string& file, const lm_model& m) {
  FsWriter fs(file);
  if (!fs.isOpened()) throw std::runtime_error("Could not write the model file: " + file + ".");
  const lm_detector* src[6] = {&m.paw_side, &m.paw_bottom, &m.tail_side, &m.tail_bottom, &m.snout_side, &m.snout_bottom};
  for (int k = 0; k < 6; ++k) {
    fs << kModelNames[k];
    fs.write_mat_d(src[k]->weights, src[k]->rows, src[k]->cols);
  }
  for (int k = 0; k < 6; ++k) fs << kModelBiases[k] << src[k]->bias;
  fs.release();
}

void load_calibration(const std::string& file, Calibration& out) {
  FsNode cal;
  if (!read_file_storage(file, cal))
    throw std::invalid_argument("Error: Could not open the calibration file: " + file + ".\n");
  const FsMat C = cal["ind_warp_mapping"].to_mat();
  if (C.empty()) throw std::invalid_argument("ind_warp_mapping is empty or undefined.");
  const FsMat V = cal["view_boxes"].to_mat();
  if (V.empty()) throw std::invalid_argument("view_boxes is empty or undefined.");
  if (V.rows != 2 || V.cols != 4) throw std::invalid_argument("view_boxes sould be a 2x4 matrix.");
  if (V.dt != 'i') throw std::invalid_argument("Bounding boxes must be defined with integer pixel positions!");
  if (C.dt != 'i') throw std::invalid_argument("ind_warp_mapping must be an integer (dt: i) matrix.");
  out.rows = C.rows;
  out.cols = C.cols;
  out.map.assign(C.v.begin(), C.v.end());
  out.side_view = lm_rect{(int)V.v[0], (int)V.v[1], (int)V.v[2], (int)V.v[3]};
  out.bottom_view = lm_rect{(int)V.v[4], (int)V.v[5], (int)V.v[6], (int)V.v[7]};
}

}  // namespace locomouse
