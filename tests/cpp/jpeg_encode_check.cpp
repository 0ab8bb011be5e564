// jpeg_encode_check.cpp — stand-alone sanitizer run of the host JPEG encoder
// (host/JpegEncode.cpp): random sizes, qualities and images, grey and colour.
// Every file must stay within the worst case include/locomouse_encode.h
// derives, and the host decoder (host/Jpeg.cpp) must take it and give back an
// image of the same size; at quality 100 a grey image comes back with a mean
// absolute error of at most one grey level.  Usage: jpeg_encode_check cases seed
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "Jpeg.hpp"
#include "JpegEncode.hpp"

using namespace locomouse;

int main(int argc, char** argv) {
  const int cases = argc > 1 ? std::atoi(argv[1]) : 100;
  std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
  int failures = 0;
  for (int k = 0; k < cases; ++k) {
    const int rows = 1 + (int)(rng() % 40), cols = 1 + (int)(rng() % 70);
    const bool colour = rng() & 1;
    const int quality = k % 7 == 0 ? 100 : 1 + (int)(rng() % 100);
    const int kind = (int)(rng() % 3);
    std::vector<uint8_t> px((size_t)rows * cols * (colour ? 3 : 1));
    for (auto& v : px) v = kind == 0 ? (uint8_t)rng() : kind == 1 ? (uint8_t)((rng() & 1) * 255) : (uint8_t)(rng() % 8 + 120);
    std::vector<uint8_t> jpg;
    encode_jpeg(px.data(), rows, cols, colour ? JpegInput::Rgb24 : JpegInput::Gray8, quality, jpg);
    const size_t nblk = colour ? 6 * (size_t)((rows + 15) / 16) * ((cols + 15) / 16) : (size_t)((rows + 7) / 8) * ((cols + 7) / 8);
    bool ok = jpg.size() <= 640 + 2 * 4 * (52 * nblk + 1) + 2;
    int r = 0, c = 0;
    std::vector<uint8_t> back;
    std::string err;
    ok = ok && decode_jpeg_channel0(jpg.data(), jpg.size(), r, c, back, &err) && r == rows && c == cols;
    if (ok && !colour && quality == 100) {
      // every table entry is 1: a coefficient is off by at most half a unit, which an orthonormal transform spreads
      // to a standard deviation of 0.29 grey levels per pixel; a mean absolute error of 1 is far outside that
      long sum = 0;
      for (size_t i = 0; i < back.size(); ++i) sum += std::abs((int)back[i] - (int)px[i]);
      ok = sum <= (long)back.size();
    }
    if (!ok) {
      ++failures;
      std::printf("case %d failed: %dx%d colour %d quality %d kind %d %s\n", k, rows, cols, (int)colour, quality, kind, err.c_str());
    }
  }
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
