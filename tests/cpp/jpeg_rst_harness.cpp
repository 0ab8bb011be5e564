// jpeg_rst_harness.cpp — test access to the device decoder's interval path on
// the host: the schedule of k_jpeg_scan_rst and the hand-over to the
// subsequence path (csrc/lm_jpeg_scan.h), lane by lane on the CPU, then DC
// sums, IDCT and channel 0 as tests/cpp/jpeg_harness.cpp runs them.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "lm_jpeg_hdr.h"
#include "lm_jpeg_scan.h"

#define JH_API extern "C" __attribute__((visibility("default")))

// As jh_lanes_decode: the frame's class (0 in scope, 1 needs host, 2 rejected;
// reason in err), or 1 when the frame is not rows x cols or the scan raised
// error bits.  stats = {1 when the interval path finished the frame, lanes it
// ran, 1 when a restart frame was handed to the subsequence path, error bits,
// nblk, longest interval in bytes}.
JH_API int jrh_intervals_decode(const uint8_t* data, size_t size, int rows, int cols, int subseq, int lanes, uint8_t* out,
                                int16_t* coef_out, int64_t coef_cap, uint32_t* stats, char* err, int errn) {
  lmj::Header h;
  std::vector<uint32_t> rst;
  lmj::parse(data, size, h, &rst);
  if (err && errn > 0) {
    std::strncpy(err, h.why.c_str(), (size_t)errn - 1);
    err[errn - 1] = 0;
  }
  if (h.cls != lmj::kInScope) return (int)h.cls;
  if (h.H != rows || h.W != cols) return 1;
  LmjTableSet T;
  lmj::make_tables(h, T);
  LmjScan sc = lmj::make_scan(h, (uint32_t)subseq);
  sc.d = data + h.scan_off;
  std::vector<int16_t> coef((size_t)sc.nblk * 64);
  std::vector<int32_t> dcd(sc.nblk);
  const uint32_t expected = lmj_expected_rst(sc);
  const bool on_path = expected > 0 && rst.size() == expected;
  const bool done = lmj_scan_intervals_host(sc, T, rst.data(), (uint32_t)rst.size(), coef.data(), dcd.data());
  uint32_t e = 0;
  if (!done) e = lmj_scan_frame_host(sc, T, lanes, coef.data(), dcd.data(), nullptr);
  if (stats) {
    stats[0] = done;
    stats[1] = on_path ? expected + 1 : 0;
    stats[2] = expected > 0 && !done;
    stats[3] = e;
    stats[4] = sc.nblk;
    stats[5] = 0;
    if (on_path) {
      uint32_t prev = 0;
      for (uint32_t off : rst) {
        if (off - 2 - prev > stats[5]) stats[5] = off - 2 - prev;
        prev = off;
      }
      if (sc.len - prev > stats[5]) stats[5] = sc.len - prev;
    }
  }
  if (e) return 1;
  lmj_dc_host(sc, coef.data(), dcd.data());
  if (coef_out && coef_cap >= (int64_t)coef.size()) std::memcpy(coef_out, coef.data(), coef.size() * sizeof(int16_t));
  const LmjPlanes P = lmj_planes(h.W, h.H, h.nc, sc.hx, sc.vx);
  std::vector<uint8_t> py((size_t)P.pitch_y * P.rows_y), pc((size_t)P.pitch_c * P.rows_c);
  for (uint32_t blk = 0; blk < sc.nblk; ++blk) {
    int comp, bx, by;
    lmj_block_pos(sc, P, blk, comp, bx, by);
    if (comp >= 2) continue;
    const int pitch = comp ? P.pitch_c : P.pitch_y;
    lmj_idct_islow(coef.data() + (size_t)blk * 64, h.qt[comp], (comp ? pc : py).data() + (size_t)by * 8 * pitch + bx * 8,
                   pitch);
  }
  for (int y = 0; y < h.H; ++y)
    for (int x = 0; x < h.W; ++x)
      out[(size_t)y * h.W + x] = lmj_channel0(py.data(), pc.data(), P, h.nc, sc.hx, sc.vx, x, y);
  return 0;
}
