// Background.cpp — see Background.hpp.
#include "Background.hpp"

#include <algorithm>
#include <stdexcept>

#include "locomouse_bkg.h"

namespace locomouse {

namespace {

struct Pinned {  // lm_host_alloc
  uint8_t* p = nullptr;
  ~Pinned() { lm_host_free(p); }
};

struct Estimator {
  lm_bkg_ctx* c = nullptr;
  ~Estimator() { lm_bkg_destroy(c); }
};

void check(lm_status s) {
  if (s != LM_OK) throw std::runtime_error(std::string("estimate_background: ") + lm_last_error());
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

}  // namespace

void parse_background_spec(const std::string& spec, BackgroundOptions& opt) {
  std::vector<std::string> part(1);
  for (char ch : spec) {
    if (ch == ':')
      part.emplace_back();
    else
      part.back().push_back(ch);
  }
  const std::string form = "LM_BACKGROUND: expected median[:stride[:permille]], not " + spec + ".";
  if (part.size() > 3 || part[0] != "median") throw std::invalid_argument(form);
  if (part.size() > 1) {
    const long s = whole_number(part[1]);
    if (s < 1) throw std::invalid_argument("LM_BACKGROUND: stride must be a whole number of at least 1, not " + part[1] + ".");
    opt.stride = (int)s;
  }
  if (part.size() > 2) {
    const long p = whole_number(part[2]);
    if (p < 0 || p > 1000) throw std::invalid_argument("LM_BACKGROUND: permille must be in 0..1000, not " + part[2] + ".");
    opt.permille = (int)p;
  }
}

void estimate_background(const LocoMouse_Inputs& in, const BackgroundOptions& opt, std::vector<uint8_t>& out) {
  const int rows = in.setup.video_rows, cols = in.setup.video_cols;
  if (rows <= 0 || cols <= 0) throw std::runtime_error("estimate_background: the video has no size");
  if (opt.stride < 1) throw std::runtime_error("estimate_background: stride must be at least 1");
  if (opt.permille < 0 || opt.permille > 1000) throw std::runtime_error("estimate_background: permille must be in 0..1000");
  if (!in.read_frames && !in.read_frame) throw std::runtime_error("estimate_background: no frame reader");
  const int64_t total = in.n_frames;
  if (total < 1) throw std::runtime_error("estimate_background: the video has no frames");
  const int64_t stride = opt.stride, sampled = (total + stride - 1) / stride;
  if (sampled > LM_BKG_MAX_SAMPLES) {
    const int64_t fits = (total + LM_BKG_MAX_SAMPLES - 1) / LM_BKG_MAX_SAMPLES;
    throw std::runtime_error("estimate_background: " + std::to_string(sampled) + " sampled frames (" +
                             std::to_string(total) + " at stride " + std::to_string(stride) + ") exceed the " +
                             std::to_string(LM_BKG_MAX_SAMPLES) + " one estimate takes; the smallest stride that fits is " +
                             std::to_string(fits) + ".");
  }
  const size_t fb = (size_t)rows * cols;
  const int batch = (int)std::min<int64_t>(std::max(opt.batch, 1), total);
  Estimator E;
  check(lm_bkg_create(opt.device, rows, cols, batch, &E.c));
  Pinned buf;
  check(lm_host_alloc(fb * (size_t)batch, reinterpret_cast<void**>(&buf.p)));
  for (int64_t first = 0; first < total;) {
    const int want = (int)std::min<int64_t>(batch, total - first);
    int got = 0;
    if (in.read_frames) {
      got = in.read_frames(buf.p, want);
    } else {
      while (got < want && in.read_frame(buf.p + (size_t)got * fb)) ++got;
    }
    if (got != want)
      throw std::runtime_error("estimate_background: failed to read frame " + std::to_string(first + std::max(got, 0)) +
                               " of " + std::to_string(total));
    // the sampled frames of this batch lie `stride` frames apart: one push at that pitch
    const int64_t skip = (stride - first % stride) % stride;
    if (skip < got) {
      const int n = (int)((got - skip + stride - 1) / stride);
      check(lm_bkg_push(E.c, buf.p + (size_t)skip * fb, (int64_t)fb * stride, n));
    }
    first += got;
  }
  out.resize(fb);
  check(lm_bkg_finish(E.c, opt.permille, out.data()));
  if (in.rewind) in.rewind();
}

}  // namespace locomouse
