// Preview.cpp — see Preview.hpp.
#include "Preview.hpp"

#include <algorithm>
#include <stdexcept>

#include "Jpeg.hpp"
#include "Media.hpp"
#include "locomouse_jpeg.h"

namespace locomouse {

namespace {

struct Pinned {  // lm_host_alloc
  uint8_t* p = nullptr;
  ~Pinned() { lm_host_free(p); }
};

struct Encoder {
  lm_enc_ctx* c = nullptr;
  ~Encoder() { lm_enc_destroy(c); }
};

struct Decoder {  // Decode::device: the context owns the frame buffer
  lm_jpeg_ctx* c = nullptr;
  ~Decoder() { lm_jpeg_destroy(c); }
};

void check(lm_status s) {
  if (s != LM_OK) throw std::runtime_error(std::string("write_preview: ") + lm_last_error());
}

// A whole, non-negative decimal number, or -1.
long whole_number(const std::string& s) {
  if (s.empty() || s.size() > 9) return -1;
  long v = 0;
  for (char ch : s) {
    if (ch < '0' || ch > '9') return -1;
    v = v * 10 + (ch - '0');
  }
  return v;
}

void add_mark(std::vector<lm_enc_mark>& out, int32_t x, int32_t y, int radius, int colour) {
  if (x < 0 || y < 0) return;
  out.push_back(lm_enc_mark{x, y, radius, colour});
}

}  // namespace

void parse_preview_spec(const std::string& spec, LocoMouse_Inputs::Preview& out) {
  // Split from the right, so the path may hold colons: the last one or two fields are taken as quality and radius
  // only when they are whole numbers.
  std::string path = spec;
  std::vector<std::string> nums;
  while (nums.size() < 2) {
    const size_t i = path.rfind(':');
    if (i == std::string::npos || whole_number(path.substr(i + 1)) < 0) break;
    nums.insert(nums.begin(), path.substr(i + 1));
    path.resize(i);
  }
  if (path.empty() || path.back() == ':')
    throw std::invalid_argument("LM_PREVIEW: expected path.avi[:quality[:radius]], not " + spec + ".");
  out.path = path;
  if (nums.size() > 0) {
    const long q = whole_number(nums[0]);
    if (q < 1 || q > 100) throw std::invalid_argument("LM_PREVIEW: quality must be in 1..100, not " + nums[0] + ".");
    out.quality = (int)q;
  }
  if (nums.size() > 1) {
    const long r = whole_number(nums[1]);
    if (r > LM_ENC_MAX_RADIUS)
      throw std::invalid_argument("LM_PREVIEW: radius must be in 0.." + std::to_string(LM_ENC_MAX_RADIUS) + ", not " +
                                  nums[1] + ".");
    out.radius = (int)r;
  }
}

void preview_marks(const TrackResults& tracks, unsigned frame, int radius, std::vector<lm_enc_mark>& out) {
  // the tail first, so that a paw on it stays visible
  const IntMat& T = tracks.tracks_tail;
  for (int t = 0; t < LM_N_TAIL_POINTS; ++t) {
    const int c = (int)frame * LM_N_TAIL_POINTS + t;
    if (T.rows < 3 || c >= T.cols) break;
    add_mark(out, T.at(0, c), T.at(1, c), kPreviewTailRadius, kPreviewTailColour);
    add_mark(out, T.at(0, c), T.at(2, c), kPreviewTailRadius, kPreviewTailColour);
  }
  auto point = [&](const IntMat& M, int colour) {
    if ((int)frame >= M.rows || M.cols < 3) return;
    const int32_t* m = M.row((int)frame);
    add_mark(out, m[0], m[1], radius, colour);
    add_mark(out, m[0], m[2], radius, colour);
  };
  for (size_t i = 0; i < tracks.paw_tracks.size() && i < 4; ++i) point(tracks.paw_tracks[i], kPreviewPawColour[i]);
  if (!tracks.snout_tracks.empty()) point(tracks.snout_tracks[0], kPreviewSnoutColour);
}

void write_preview(const LocoMouse_Inputs& in, const TrackResults& tracks, unsigned n_frames, int fps) {
  const int rows = in.setup.video_rows, cols = in.setup.video_cols;
  const int crows = in.setup.calib_rows, ccols = in.setup.calib_cols;
  if (in.preview.path.empty()) throw std::runtime_error("write_preview: no path");
  if (rows <= 0 || cols <= 0 || crows <= 0 || ccols <= 0) throw std::runtime_error("write_preview: the video has no size");
  if (!in.read_frames && !in.read_frame) throw std::runtime_error("write_preview: no frame reader");
  const bool on_device = in.decode == LocoMouse_Inputs::Decode::device;
  if (on_device && !in.read_compressed) throw std::runtime_error("write_preview: Decode::device needs read_compressed");
  const int device = in.devices.empty() ? in.device : in.devices[0];
  const size_t fb = (size_t)rows * cols;
  // as many frames per call as the encoder's 2^31 bytes of worst-case output allow
  const int64_t slot = lm_enc_slot_bytes(crows, ccols, LM_ENC_RGB24);
  if (slot < 0) throw std::runtime_error("write_preview: the corrected image is too large to encode");
  const int64_t fit = std::min<int64_t>(((int64_t)1 << 31) / slot - 1, LM_ENC_MAX_BATCH);
  if (fit < 1) throw std::runtime_error("write_preview: the corrected image is too large to encode");
  const int batch = (int)std::min<int64_t>({(int64_t)std::max(in.batch, 1), fit, (int64_t)n_frames});
  if (batch < 1) throw std::runtime_error("write_preview: the video has no frames");

  Encoder E;
  check(lm_enc_create(device, crows, ccols, LM_ENC_RGB24, in.preview.quality, batch, &E.c));
  lm_enc_overlay geo{in.setup.ind_warp_mapping, rows, cols, crows, ccols, in.setup.flip, 0};
  check(lm_enc_set_overlay(E.c, &geo));
  Decoder D;
  uint8_t* d_frames = nullptr;
  Pinned buf;
  if (on_device) {
    check(lm_jpeg_create(device, rows, cols, batch, 0, &D.c));
    check(lm_jpeg_device_alloc(D.c, fb * (size_t)batch, &d_frames));
  } else {
    check(lm_host_alloc(fb * (size_t)batch, reinterpret_cast<void**>(&buf.p)));
  }
  MjpegAviWriter avi;
  if (!avi.open(in.preview.path, crows, ccols, fps > 0 ? fps : 30))
    throw std::runtime_error("write_preview: could not create " + in.preview.path + ".");
  if (in.rewind) in.rewind();
  std::vector<lm_enc_mark> marks;
  std::vector<int32_t> mark_offset;
  std::vector<std::vector<uint8_t>> jpegs;
  std::vector<uint8_t> tmp;
  for (unsigned first = 0; first < n_frames;) {
    const int want = (int)std::min<unsigned>((unsigned)batch, n_frames - first);
    marks.clear();
    mark_offset.assign(1, 0);
    for (int i = 0; i < want; ++i) {
      preview_marks(tracks, first + (unsigned)i, in.preview.radius, marks);
      mark_offset.push_back((int32_t)marks.size());
    }
    lm_enc_result res{};
    int got = 0;
    if (on_device) {
      jpegs.clear();
      got = in.read_compressed(jpegs, want);
      if (got == want) {
        std::vector<const uint8_t*> ptr((size_t)want);
        std::vector<size_t> size((size_t)want);
        std::vector<int32_t> status((size_t)want);
        for (int i = 0; i < want; ++i) {
          ptr[i] = jpegs[i].data();
          size[i] = jpegs[i].size();
          if (!size[i]) throw std::runtime_error("write_preview: failed to read frame " + std::to_string(first + i));
        }
        check(lm_jpeg_decode_device(D.c, ptr.data(), size.data(), want, d_frames, (int64_t)fb, status.data()));
        for (int i = 0; i < want; ++i) {  // a frame the device hands back is decoded here, as in the detection pass
          if (status[i] == LM_JPEG_OK) continue;
          tmp.resize(fb);
          if (!decode_jpeg_channel0_into(ptr[i], size[i], rows, cols, tmp.data()))
            throw std::runtime_error("write_preview: failed to decode frame " + std::to_string(first + i));
          check(lm_jpeg_upload(D.c, d_frames + (size_t)i * fb, tmp.data(), fb));
        }
        check(lm_enc_render_encode_device(E.c, d_frames, (int64_t)fb, want, marks.data(), mark_offset.data(), &res));
      }
    } else {
      if (in.read_frames) {
        got = in.read_frames(buf.p, want);
      } else {
        while (got < want && in.read_frame(buf.p + (size_t)got * fb)) ++got;
      }
      if (got == want) check(lm_enc_render_encode(E.c, buf.p, (int64_t)fb, want, marks.data(), mark_offset.data(), &res));
    }
    if (got != want)
      throw std::runtime_error("write_preview: failed to read frame " + std::to_string(first + (unsigned)std::max(got, 0)) +
                               " of " + std::to_string(n_frames));
    for (int i = 0; i < want; ++i) {
      if (!avi.fits(res.size[i])) {  // an AVI's sizes are 32 bits: keep what fits as a whole file, and say so
        const uint32_t kept = avi.frame_count();
        avi.close();
        throw std::runtime_error("write_preview: " + in.preview.path + " reached the 4 GiB an AVI file holds after " +
                                 std::to_string(kept) + " of " + std::to_string(n_frames) +
                                 " frames; it is complete up to there.  A lower quality fits more frames.");
      }
      if (!avi.add(res.data + res.offset[i], res.size[i]))
        throw std::runtime_error("write_preview: could not write " + in.preview.path + " (frame " +
                                 std::to_string(first + (unsigned)i) + ").");
    }
    first += (unsigned)want;
  }
  if (!avi.close()) throw std::runtime_error("write_preview: could not write " + in.preview.path + ".");
  if (in.rewind) in.rewind();
}

}  // namespace locomouse
