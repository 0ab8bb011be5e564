// VideoFrames.hpp — the frame source the programs (LocoMouse, LocoMouseBackground)
// put behind LocoMouse_Inputs::read_frame / read_frames / read_compressed / rewind.
#ifndef LOCOMOUSE_HOST_VIDEOFRAMES_HPP
#define LOCOMOUSE_HOST_VIDEOFRAMES_HPP

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <memory>
#include <thread>
#include <vector>

#include "Media.hpp"

namespace locomouse {

// V >> F in video order; a whole batch at a time is decoded straight into
// the caller's batch buffer by worker threads (pread at each frame's offset
// in the file), so decoding is parallel and costs no extra copy.
class VideoFrames {
 public:
  VideoFrames(std::shared_ptr<AviReader> v, int threads)
      : V(std::move(v)), T(threads), FB((size_t)V->rows() * V->cols()) {}
  bool read(uint8_t* dst) { return pos < V->frame_count() && V->read_at(pos++, dst); }
  int read(uint8_t* dst, int n) {
    const auto t0 = std::chrono::steady_clock::now();
    n = (int)std::min<size_t>((size_t)std::max(n, 0), V->frame_count() - pos);
    std::vector<char> ok((size_t)n, 0);
    std::atomic<int> next{0};
    auto work = [&] {
      for (int i; (i = next++) < n;) ok[i] = V->read_at(pos + (size_t)i, dst + (size_t)i * FB) ? 1 : 0;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(T, n); ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    int got = 0;
    while (got < n && ok[got]) ++got;
    pos += (size_t)got;
    decode_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return got;
  }
  // The next (up to) n frames' chunks as they are in the file (JPEG images of an MJPEG video), appended to out.
  int read_compressed(std::vector<std::vector<uint8_t>>& out, int n) {
    n = (int)std::min<size_t>((size_t)std::max(n, 0), V->frame_count() - pos);
    int got = 0;
    for (; got < n; ++got) {
      std::vector<uint8_t> b;
      if (!V->read_chunk(pos + (size_t)got, b)) break;
      out.push_back(std::move(b));
    }
    pos += (size_t)got;
    return got;
  }
  int threads() const { return T; }
  double decode_s = 0;  // wall seconds in read(dst, n): file reads + decoding on T threads
  void rewind() { pos = 0; }  // V.set(CV_CAP_PROP_POS_FRAMES, 0)

 private:
  std::shared_ptr<AviReader> V;
  const int T;
  const size_t FB;
  size_t pos = 0;
};

}  // namespace locomouse

#endif
