// bkg_harness.cpp — what the background tests need from C++ without a GPU:
// the host statement of csrc/lm_bkg_core.h (accumulate + select with the code
// the kernels run) and host/Media.cpp's PNG writer and reader.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "Media.hpp"
#include "lm_bkg_core.h"

extern "C" {

// Frames pushed in `npush` pushes of sizes push_n[k] (frame i at frames + i * pitch); out: npix bytes.
int bh_median(const uint8_t* frames, int64_t pitch, const int32_t* push_n, int32_t npush, int64_t npix, int32_t permille,
              uint8_t* out) {
  std::vector<lmb_count> hist((size_t)npix * LMB_BINS, 0);
  int64_t samples = 0;
  for (int32_t k = 0; k < npush; ++k) {
    if (samples + push_n[k] > LMB_MAX_SAMPLES) return 1;
    lmb_host_accumulate(hist.data(), frames + samples * pitch, pitch, push_n[k], (size_t)npix);
    samples += push_n[k];
  }
  if (samples < 1) return 2;
  lmb_host_select(hist.data(), (size_t)npix, permille, samples, out);
  return 0;
}

uint32_t bh_rank(int32_t permille, int64_t K) { return lmb_rank(permille, K); }
int32_t bh_max_samples() { return LMB_MAX_SAMPLES; }

int bh_write_png(const char* path, int rows, int cols, const uint8_t* pixels) {
  return locomouse::write_png_gray(path, rows, cols, pixels) ? 0 : 1;
}

int bh_read_png(const char* path, int* rows, int* cols, uint8_t* out, int64_t cap) {
  std::vector<uint8_t> px;
  if (!locomouse::read_png_gray(path, *rows, *cols, px)) return 1;
  if ((int64_t)px.size() > cap) return 2;
  std::memcpy(out, px.data(), px.size());
  return 0;
}
}
