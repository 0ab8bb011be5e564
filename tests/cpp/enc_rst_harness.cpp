// enc_rst_harness.cpp — C entry point for the tests of the host JPEG encoder's
// restart intervals (host/JpegEncode.cpp).  Links no GPU library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "JpegEncode.hpp"

using namespace locomouse;

extern "C" {

// The JPEG file of one image with a restart interval (in MCUs) into out (cap
// bytes); its size, -1 for an exception (message in err), -2 when it does not fit.
int64_t erh_encode(const uint8_t* px, int rows, int cols, int format, int quality, int restart_interval, uint8_t* out,
                   int64_t cap, char* err, int errn) {
  try {
    std::vector<uint8_t> j;
    encode_jpeg(px, rows, cols, (JpegInput)format, quality, j, restart_interval);
    if ((int64_t)j.size() > cap) return -2;
    std::memcpy(out, j.data(), j.size());
    return (int64_t)j.size();
  } catch (const std::exception& e) {
    if (err && errn > 0) std::snprintf(err, (size_t)errn, "%s", e.what());
    return -1;
  }
}

}  // extern "C"
