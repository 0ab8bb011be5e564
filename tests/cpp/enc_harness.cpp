// enc_harness.cpp — C entry points for the tests of the host JPEG encoder
// (host/JpegEncode.cpp) and the MJPEG AVI writer (host/Media.cpp).  Links no
// GPU library.
#include <cstdint>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "JpegEncode.hpp"
#include "Media.hpp"

using namespace locomouse;

extern "C" {

// The JPEG file of one image into out (cap bytes); its size, -1 for an
// exception (message in err), -2 when it does not fit.
int64_t eh_encode(const uint8_t* px, int rows, int cols, int format, int quality, uint8_t* out, int64_t cap, char* err,
                  int errn) {
  try {
    std::vector<uint8_t> j;
    encode_jpeg(px, rows, cols, (JpegInput)format, quality, j);
    if ((int64_t)j.size() > cap) return -2;
    std::memcpy(out, j.data(), j.size());
    return (int64_t)j.size();
  } catch (const std::exception& e) {
    if (err && errn > 0) std::snprintf(err, (size_t)errn, "%s", e.what());
    return -1;
  }
}

// Blocks in scan order, 64 zig-zag int16 each; the block count, -1 / -2 as above.
int64_t eh_coefficients(const uint8_t* px, int rows, int cols, int format, int quality, int16_t* out, int64_t cap) {
  try {
    std::vector<int16_t> c;
    encode_jpeg_coefficients(px, rows, cols, (JpegInput)format, quality, c);
    if ((int64_t)c.size() > cap) return -2;
    std::memcpy(out, c.data(), c.size() * sizeof(int16_t));
    return (int64_t)c.size() / 64;
  } catch (const std::exception&) {
    return -1;
  }
}

// n frames (tightly packed, one after another) encoded on `threads` host threads, each taking the next frame not yet
// taken; the files' total size, or -1.  For rate measurements (scripts/preview_rate.py).
int64_t eh_encode_many(const uint8_t* px, int rows, int cols, int format, int quality, int n, int threads) {
  const size_t fb = (size_t)rows * cols * (format == 1 ? 3 : 1);
  std::atomic<int> next{0};
  std::atomic<int64_t> total{0};
  std::atomic<bool> failed{false};
  auto work = [&] {
    std::vector<uint8_t> j;
    for (int i = next++; i < n; i = next++) {
      j.clear();
      try {
        encode_jpeg(px + (size_t)i * fb, rows, cols, (JpegInput)format, quality, j);
      } catch (const std::exception&) {
        failed = true;
        return;
      }
      total += (int64_t)j.size();
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  return failed ? -1 : total.load();
}

int eh_write_avi(const char* path, const uint8_t* const* jpegs, const size_t* sizes, int n, int rows, int cols, int fps) {
  MjpegAviWriter w;
  if (!w.open(path, rows, cols, fps)) return 1;
  for (int i = 0; i < n; ++i)
    if (!w.add(jpegs[i], sizes[i])) return 2;
  if ((int)w.frame_count() != n) return 3;
  return w.close() ? 0 : 4;
}

// info: rows, cols, frames, fps, is_mjpeg
int eh_avi_info(const char* path, int32_t* info) {
  AviReader r;
  if (!r.open(path)) return 1;
  info[0] = r.rows();
  info[1] = r.cols();
  info[2] = (int32_t)r.frame_count();
  info[3] = r.fps();
  info[4] = r.is_mjpeg();
  return 0;
}

int64_t eh_avi_chunk(const char* path, int index, uint8_t* out, int64_t cap) {
  AviReader r;
  std::vector<uint8_t> b;
  if (!r.open(path) || !r.read_chunk((size_t)index, b)) return -1;
  if ((int64_t)b.size() > cap) return -2;
  std::memcpy(out, b.data(), b.size());
  return (int64_t)b.size();
}

// Every frame's channel 0 through AviReader::read, in order (rows * cols bytes each); the frames read.
int eh_avi_frames(const char* path, uint8_t* out, int max_frames) {
  AviReader r;
  if (!r.open(path)) return -1;
  int n = 0;
  while (n < max_frames && r.read(out + (size_t)n * r.rows() * r.cols())) ++n;
  return n;
}

}  // extern "C"
