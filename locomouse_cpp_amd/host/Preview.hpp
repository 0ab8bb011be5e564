// Preview.hpp — the annotated preview video: every frame of the
// video as the detector's geometry sees it (the corrected, optionally flipped
// image, without background subtraction), with the exported paw, snout and
// tail tracks drawn on it, rendered and JPEG-encoded on the device
// (include/locomouse_encode.h) and written as an MJPEG AVI.  The reference
// leaves looking at its results to the MATLAB GUI.  Not in the reference.
#ifndef LOCOMOUSE_HOST_PREVIEW_HPP
#define LOCOMOUSE_HOST_PREVIEW_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "LocoMouse.hpp"
#include "locomouse_encode.h"

namespace locomouse {

// Colour indices (LM_ENC_PALETTE) of the features: paw tracks 0..3, the snout, the tail.
constexpr int kPreviewPawColour[4] = {0, 1, 2, 3};
constexpr int kPreviewSnoutColour = 4;
constexpr int kPreviewTailColour = 5;
constexpr int kPreviewTailRadius = 1;

// "path.avi[:quality[:radius]]" (the LM_PREVIEW knob) into `out`; quality in
// 1..100 (default 90), radius in 0..LM_ENC_MAX_RADIUS (default 3).  The fields
// are split off from the right and only when they are whole numbers, so the
// path may contain colons (a path that itself ends in ":<number>" needs the
// quality spelled out behind it).  Throws std::invalid_argument("LM_PREVIEW:
// ...") for anything else.
void parse_preview_spec(const std::string& spec, LocoMouse_Inputs::Preview& out);

// Frame f's marks from the exported tracks, appended to `out`.  The exported
// coordinates are zero-based column / row indices into the corrected image
// (Tracks.cpp exportPointTracks: corner - size + 1 is the crop's first column
// and the candidate's coordinate counts from 0 inside it), which is the
// canvas, so a mark is centred on the pixel the coordinate names.  Each paw
// and the snout give a mark at (m[0], m[1]) in the bottom view and, when
// m[2] >= 0, at (m[0], m[2]) in the side view; the 15 tail points likewise
// with radius 1.  A coordinate of -1 draws nothing.
void preview_marks(const TrackResults& tracks, unsigned frame, int radius, std::vector<lm_enc_mark>& out);

// One more pass over the video (in.rewind first and last): frames reach the
// device as they do for detection (read_frames / read_frame and an upload, or
// read_compressed and lm_jpeg_decode_device when in.decode is Decode::device),
// are rendered and encoded in batches of in.batch on the first device, and the
// AVI is written to in.preview.path at `fps` frames per second.  Throws
// std::runtime_error.  An AVI file holds 4 GiB (about 45,000 frames of
// 1024 x 256 at quality 90, at 94 KB a frame): a longer preview stops there with an error that
// says how many frames it holds, and the file is complete up to that frame.
void write_preview(const LocoMouse_Inputs& in, const TrackResults& tracks, unsigned n_frames, int fps);

}  // namespace locomouse

#endif
