// Cli.cpp — the `LocoMouse` executable: the same
// command line, files, output and exit codes as the reference's CLI, over the
// host mirror and the MI355X C-ABI.
//
//   LocoMouse <method> config.yml video.avi background.png model.yml calibration.yml L|R output_folder
//
// Reference: main.cpp:38-105 (sequence, messages, exit codes),
// LocoMouse_ParseInputs.cpp:1-99 (arguments, calibration file),
// LocoMouse_class.cpp:12-249 (config.yml), :294-540 (constructor: video,
// background, sizes, flip, output file), :3095-3162 (model file).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <atomic>
#include <cstring>
#include <thread>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Background.hpp"
#include "FileStorage.hpp"
#include "Inputs.hpp"
#include "LocoMouse.hpp"
#include "Media.hpp"
#include "Preview.hpp"
#include "VideoFrames.hpp"

namespace locomouse {
namespace {

struct ParsedInputs {  // LocoMouse_ParseInputs
  std::string LM_CALL, CONFIG_FILE, VIDEO_FILE, BKG_FILE, MODEL_FILE, CALIBRATION_FILE, FLIP_CHAR, OUTPUT_PATH,
      METHOD, REF_PATH, FILE_STEM;
  std::vector<int32_t> CALIBRATION;
  int calib_rows = 0, calib_cols = 0;
  lm_rect BB_SIDE_VIEW{}, BB_BOTTOM_VIEW{};
};

std::string dir_of(const std::string& p) {  // dirname(3)
  size_t i = p.find_last_of('/');
  if (i == std::string::npos) return ".";
  if (i == 0) return "/";
  return p.substr(0, i);
}

std::string strip_file_name(const std::string& s) {  // ParseInputs.cpp stripFileName
  std::string out;
  size_t i = s.rfind('/');
  if (i != std::string::npos) out = s.substr(i + 1);
  return out.substr(0, out.find_last_of('.'));
}

ParsedInputs parse_inputs(int argc, char** argv) {
  ParsedInputs in;
  in.LM_CALL = argv[0];
  if (argc != 9) {
    std::cout << "Warning: Invalid input list. The input should be: LocoMouse method config.yml video.avi "
                 "background.png model_file.yml calibration_file.yml side_char output_folder."
              << std::endl;
    std::cout << "Attempting to run with default paramters..." << std::endl;
    in.REF_PATH = dir_of(argv[0]) + "/";
    in.FILE_STEM = "L7Y9_control1_L";
    in.CONFIG_FILE = in.REF_PATH + "config.yml";
    in.VIDEO_FILE = in.REF_PATH + "L7Y9_control1_L.avi";
    in.BKG_FILE = in.REF_PATH + "L7Y9_control1_L.png";
    in.MODEL_FILE = in.REF_PATH + "model_LocoMouse_paper.yml";
    in.CALIBRATION_FILE = in.REF_PATH + "IDX_pen_correct_fields2.yml";
    in.FLIP_CHAR = "L";
    in.OUTPUT_PATH = in.REF_PATH + ".";
    in.METHOD = "0";
  } else {
    in.VIDEO_FILE = argv[3];
    in.CONFIG_FILE = argv[2];
    in.REF_PATH = dir_of(argv[0]) + "/";
    in.FILE_STEM = strip_file_name(in.VIDEO_FILE);
    in.MODEL_FILE = argv[5];
    in.BKG_FILE = argv[4];
    in.CALIBRATION_FILE = argv[6];
    in.FLIP_CHAR = argv[7];
    in.OUTPUT_PATH = argv[8];
    in.METHOD = argv[1];
  }
  Calibration cal;
  load_calibration(in.CALIBRATION_FILE, cal);
  in.calib_rows = cal.rows;
  in.calib_cols = cal.cols;
  in.CALIBRATION = std::move(cal.map);
  in.BB_SIDE_VIEW = cal.side_view;
  in.BB_BOTTOM_VIEW = cal.bottom_view;
  return in;
}

int run(int argc, char** argv) {
  ParsedInputs in = parse_inputs(argc, argv);
  LocoMouse_Inputs li;
  const int method = std::stoi(in.METHOD);  // LocoMouse::initializePaths
  DebugConfig dbg;
  // LM_REFERENCE_BRIGHTNESS=intended (not in the reference): use_reference_image_brightness as the reference
  // means it (LocoMouse_Inputs::reference_intended); unset or empty: as it executes it, which cannot start
  if (const char* rb = std::getenv("LM_REFERENCE_BRIGHTNESS")) {
    const std::string v = rb;
    if (v == "intended") li.reference_intended = true;
    else if (!v.empty()) throw std::invalid_argument("LM_REFERENCE_BRIGHTNESS: must be intended, not " + v + ".");
  }
  ReferenceImage ref_image;
  load_config(in.CONFIG_FILE, in.REF_PATH, li.params, li.bb_params, dbg, &ref_image);
  li.reference_rows = ref_image.rows;
  li.reference_cols = ref_image.cols;
  li.reference_image = std::move(ref_image.px);
  auto video = std::make_shared<AviReader>();
  if (!video->open(in.VIDEO_FILE)) throw std::invalid_argument("Could not open the video file: " + in.VIDEO_FILE + ".");
  li.n_frames = video->frame_count();
  if (dbg.verbose && dbg.n_frames > 0)  // loadVideo (:380-389): debugging runs the first N_debug_frames only
    li.n_frames = std::min<uint32_t>(li.n_frames, (uint32_t)dbg.n_frames);
  li.verbose_debug = dbg.verbose;
  li.debug_file = in.OUTPUT_PATH + "/debug_" + in.FILE_STEM + ".yml";  // initializePaths (:361-362)
  li.debug_text = in.OUTPUT_PATH + "/debug_" + in.FILE_STEM + ".txt";
  if (li.n_frames < 1) throw std::invalid_argument("Error: Video has no images to read from.");
  // LM_BACKGROUND=median[:stride[:permille]] (not in the reference): the background is estimated from the
  // video (Background.hpp) once the frame reader below exists, and the background argument is not opened
  BackgroundOptions bkg_opt;
  const char* bkg_spec = std::getenv("LM_BACKGROUND");
  if (bkg_spec) parse_background_spec(bkg_spec, bkg_opt);
  // LM_PREVIEW=path.avi[:quality[:radius]] (not in the reference): after the results are exported, the annotated
  // preview video is written there (Preview.hpp)
  if (const char* pv = std::getenv("LM_PREVIEW"))
    if (*pv) parse_preview_spec(pv, li.preview);  // set but empty means off, as for LM_DECODE
  int br = 0, bc = 0;
  std::vector<uint8_t> bkg;
  if (!bkg_spec && !read_png_gray(in.BKG_FILE, br, bc, bkg))
    throw std::invalid_argument("Could not open the background image: " + in.BKG_FILE + ".");
  if (!bkg_spec && (bc != video->cols() || br != video->rows())) {  // validateImageVideoSize (:486-492)
    std::ostringstream m;
    m << "Error: Background image does not match video size. Background image has size [" << bc << " x " << br
      << "] while Video has size [" << video->cols() << " x " << video->rows() << "]." << '\n';
    throw std::runtime_error(m.str());
  }
  Model model;
  load_model(in.MODEL_FILE, model);
  if (in.FLIP_CHAR.size() != 1 || (in.FLIP_CHAR[0] != 'L' && in.FLIP_CHAR[0] != 'R'))
    throw std::invalid_argument("Mouse side option must be either \"L\" or \"R\".");
  li.setup.method = method;
  li.setup.flip = in.FLIP_CHAR[0] == 'L';
  li.setup.video_rows = video->rows();
  li.setup.video_cols = video->cols();
  li.setup.background = bkg.data();
  li.setup.calib_rows = in.calib_rows;
  li.setup.calib_cols = in.calib_cols;
  li.setup.ind_warp_mapping = in.CALIBRATION.data();
  li.setup.view_box_side = in.BB_SIDE_VIEW;
  li.setup.view_box_bottom = in.BB_BOTTOM_VIEW;
  li.model = model.m;
  // Decode threads: MJPEG frames decode at a few hundred per second per core,
  // so a batch is spread over up to 16 (LM_READ_THREADS overrides).
  int read_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  if (const char* t = std::getenv("LM_READ_THREADS")) read_threads = std::max(1, std::atoi(t));
  auto reader = std::make_shared<VideoFrames>(video, read_threads);
  li.read_frame = [reader](uint8_t* dst) { return reader->read(dst); };
  li.read_frames = [reader](uint8_t* dst, int n) { return reader->read(dst, n); };
  li.rewind = [reader] { reader->rewind(); };
  // LM_DECODE=host|device: where MJPEG frames are decoded (LocoMouse_Inputs::decode); unset means host
  if (const char* dm = std::getenv("LM_DECODE")) {
    const std::string v = dm;
    if (v == "device") {
      if (!video->is_mjpeg())
        throw std::invalid_argument("LM_DECODE=device needs an MJPEG video (MJPG / JPEG / AVI1): " + in.VIDEO_FILE +
                                    " is not one.");
      li.decode = LocoMouse_Inputs::Decode::device;
      li.read_compressed = [reader](std::vector<std::vector<uint8_t>>& out, int n) {
        return reader->read_compressed(out, n);
      };
    } else if (v != "host" && !v.empty()) {
      throw std::invalid_argument("LM_DECODE must be host or device, not " + v + ".");
    }
  }
  li.output_file = in.OUTPUT_PATH + "/output_" + in.FILE_STEM + ".yml";
  if (const char* d = std::getenv("LM_DEVICE")) li.device = std::atoi(d);
  // LM_DEVICES=0,1,...: detection sharded over these GPUs (LocoMouse_Inputs::devices);
  // LM_OVERSUBSCRIBE=1 lets a device appear more than once (rehearsals on fewer GPUs)
  if (const char* ds = std::getenv("LM_DEVICES")) {
    std::stringstream ss(ds);
    std::string tok;
    while (std::getline(ss, tok, ','))
      if (!tok.empty()) {
        size_t used = 0;
        int d = -1;
        try {
          d = std::stoi(tok, &used);
        } catch (const std::exception&) {
          used = 0;
        }
        if (used != tok.size()) throw std::invalid_argument("LM_DEVICES: not a device index: " + tok);
        li.devices.push_back(d);
      }
  }
  if (const char* o = std::getenv("LM_OVERSUBSCRIBE")) li.oversubscribe = std::atoi(o) != 0;
  if (const char* b = std::getenv("LM_BATCH")) li.batch = std::max(1, std::atoi(b));
  if (const char* l = std::getenv("LM_LANES")) li.lanes = std::max(1, std::atoi(l));
  double background_ms = 0;
  if (bkg_spec) {  // before anything else reads the video; the pass rewinds it
    const auto t0 = std::chrono::steady_clock::now();
    bkg_opt.device = li.devices.empty() ? li.device : li.devices[0];
    bkg_opt.batch = li.batch;
    estimate_background(li, bkg_opt, bkg);
    li.setup.background = bkg.data();
    background_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (const char* save = std::getenv("LM_BACKGROUND_SAVE"))  // the image in use, estimated or loaded
    if (!write_png_gray(save, video->rows(), video->cols(), bkg.data()))
      throw std::runtime_error(std::string("Could not write the background image: ") + save + ".");
  if (std::getenv("LM_PRINT_INPUTS")) {  // diagnostics: the parsed inputs, nothing run on the GPU (but LM_BACKGROUND's pass above)
    const lm_params& P = li.params;
    std::cout << "method " << method << "\nflip " << li.setup.flip << "\nvideo " << li.setup.video_rows << " "
              << li.setup.video_cols << " " << li.n_frames << "\ncalib " << in.calib_rows << " " << in.calib_cols
              << "\noutput " << li.output_file << "\nconn " << P.conn_comp_connectivity << "\nmax_disp "
              << P.max_displacement_bottom << " " << P.max_displacement_side << "\nong_spacing "
              << P.occlusion_grid_spacing_pixels_side << " " << P.occlusion_grid_spacing_pixels_bottom
              << "\nuse_bb " << P.use_provided_bounding_box << "\nbb_side " << P.bounding_box_side.x << " "
              << P.bounding_box_side.y << " " << P.bounding_box_side.width << " " << P.bounding_box_side.height
              << "\nbb_bottom " << P.bounding_box_bottom.x << " " << P.bounding_box_bottom.y << " "
              << P.bounding_box_bottom.width << " " << P.bounding_box_bottom.height << "\nbb_params "
              << li.bb_params.median_filter_size << " " << li.bb_params.min_pixel_visible << " "
              << li.bb_params.moving_average_window << "\n";
    std::cout.precision(17);
    std::cout << "doubles " << P.side_bottom_min_overlap << " " << P.occlusion_grid_max_width << " "
              << P.tail_sub_bounding_box << " " << P.alpha_vel_bottom << " " << P.alpha_vel_side << " "
              << P.pairwise_occluded_cost << "\nprior";
    for (int r = 0; r < 5; ++r)
      for (double v : {P.location_prior[r].x, P.location_prior[r].y, P.location_prior[r].max_distance,
                       P.location_prior[r].min_x, P.location_prior[r].max_x, P.location_prior[r].min_y,
                       P.location_prior[r].max_y})
        std::cout << " " << v;
    const lm_detector* dets[6] = {&li.model.paw_bottom, &li.model.paw_side, &li.model.snout_bottom,
                                  &li.model.snout_side, &li.model.tail_bottom, &li.model.tail_side};
    for (const lm_detector* d : dets) {
      double sum = 0;
      for (int k = 0; k < d->rows * d->cols; ++k) sum += d->weights[k];
      std::cout << "\ndetector " << d->rows << " " << d->cols << " " << d->bias << " " << sum;
    }
    unsigned long long bsum = 0;
    for (uint8_t v : bkg) bsum += v;
    std::cout << "\nbackground_sum " << bsum;
    if (P.use_reference_image_brightness) {  // the reference image as the inputs carry it, and whether it will be used
      unsigned long long rsum = 0;
      for (uint8_t v : li.reference_image) rsum += v;
      std::cout << "\nreference " << (li.reference_intended ? "intended " : "as_executed ") << li.reference_rows << " "
                << li.reference_cols << " " << rsum;
    }
    std::cout << std::endl;
    return EXIT_SUCCESS;
  }
  {  // OUTPUT = FileStorage(output_file, WRITE) must open (:333-337)
    std::FILE* f = std::fopen(li.output_file.c_str(), "w");
    if (!f) throw std::runtime_error("Could not create output file:  " + li.output_file + "\n");
    std::fclose(f);
  }

  const auto t_start = std::chrono::steady_clock::now();
  std::unique_ptr<LocoMouse> L = LocoMouse_Initialize(li);  // main.cpp:45-91
  L->getBoundingBox();
  L->initializeFeatureLoop();
  const auto t_init = std::chrono::steady_clock::now();
  const double decode_init = reader->decode_s;  // the bounding-box pass's reads, when it runs
  for (unsigned int i = 0; i < L->N_frames(); ++i) {
    L->readFrame();
    L->cropBoundingBox();
    L->detectTail();
    L->detectBottomCandidates();
    L->computeUnaryCostsBottom();
    L->computePairwiseCostsBottom();
    L->detectSideCandidates();
    L->matchBottomSideCandidates();
    L->storePreviousImage();
  }
  const auto t_loop = std::chrono::steady_clock::now();
  L->computeBottomTracks();
  L->computeSideTracks();
  const auto t_tracks = std::chrono::steady_clock::now();
  L->exportResults();
  const auto t_export = std::chrono::steady_clock::now();
  const double decode_run = reader->decode_s;  // the reads up to here; the preview pass reads the video once more
  double preview_ms = 0;
  if (!li.preview.path.empty()) {  // one more pass over the video, on the first device
    write_preview(li, L->tracks(), L->N_frames(), video->fps() > 0 ? video->fps() : 30);
    preview_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_export).count();
  }
  if (std::getenv("LM_TIMING")) {  // stage times (not in the reference)
    const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const LocoMouse::StageTimes st = L->stage_times();
    std::cout << "LM_TIMING init_ms " << ms(t_start, t_init) << " loop_ms " << ms(t_init, t_loop) << " tracks_ms "
              << ms(t_loop, t_tracks) << " export_ms " << ms(t_tracks, t_export)
              << " decode_ms " << 1e3 * (decode_run - decode_init) << " decode_threads " << reader->threads()
              << " submit_ms " << 1e3 * st.submit_s << " wait_ms " << 1e3 * st.wait_s << " batches " << st.batches
              << " frames " << L->N_frames() << " decode_device_ms " << 1e3 * st.decode_device_s
              << " decode_fallback_frames " << st.decode_fallback_frames << " background_ms " << background_ms
              << " preview_ms " << preview_ms << " preview_decode_ms " << 1e3 * (reader->decode_s - decode_run)
              << std::endl;
  }
  return EXIT_SUCCESS;
}

}  // namespace
}  // namespace locomouse

int main(int argc, char* argv[]) {
  const auto t0 = std::chrono::steady_clock::now();
  int return_val = EXIT_SUCCESS;
  try {
    return_val = locomouse::run(argc, argv);
  } catch (const std::invalid_argument& e) {
    std::cout << "Invalid inputs: " << e.what() << std::endl;
    return_val = EXIT_FAILURE;
  } catch (const std::runtime_error& e) {
    std::cout << "Runtime Error: " << e.what() << std::endl;
    return_val = EXIT_FAILURE;
  }
  const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << "Total Elapsed time: " << t << "s" << std::endl;
  return return_val;
}
