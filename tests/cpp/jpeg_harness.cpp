// jpeg_harness.cpp — test access to the JPEG decoders on the host:
//   jh_host_decode   the project's host decoder (host/Jpeg.cpp), the expected bytes;
//   jh_lanes_decode  the device decoder's code (csrc/lm_jpeg_scan.h) run lane
//                    by lane on the CPU with the kernel's schedule: header
//                    parse, subsequence scan, DC sums, IDCT, channel 0.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "Jpeg.hpp"
#include "lm_jpeg_hdr.h"
#include "lm_jpeg_scan.h"

#define JH_API extern "C" __attribute__((visibility("default")))

// 0 = decoded; 1 = rejected (message in err).
JH_API int jh_host_decode(const uint8_t* data, size_t size, int rows, int cols, uint8_t* out, char* err, int errn) {
  std::string why;
  if (locomouse::decode_jpeg_channel0_into(data, size, rows, cols, out, &why)) return 0;
  if (err && errn > 0) {
    std::strncpy(err, why.c_str(), (size_t)errn - 1);
    err[errn - 1] = 0;
  }
  return 1;
}

// Returns the frame's class (0 in scope, 1 needs host, 2 rejected; reason in
// err), or 1 when the frame is not rows x cols or the scan raised error bits
// (stats[3]).  In scope: `out` gets
// rows x cols channel-0 bytes, coef (may be NULL) nblk * 64 coefficients in
// scan order, stats = {subsequences, rounds, max chunk rounds, error bits, nblk}.
JH_API int jh_lanes_decode(const uint8_t* data, size_t size, int rows, int cols, int subseq, int lanes, uint8_t* out,
                           int16_t* coef_out,
                           int64_t coef_cap, uint32_t* stats, char* err, int errn) {
  lmj::Header h;
  lmj::parse(data, size, h);
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
  LmjScanStats st;
  const uint32_t e = lmj_scan_frame_host(sc, T, lanes, coef.data(), dcd.data(), &st);
  if (stats) {
    stats[0] = st.subsequences;
    stats[1] = st.rounds;
    stats[2] = st.max_rounds;
    stats[3] = e;
    stats[4] = sc.nblk;
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

// The host decoder's own coefficients (Decoder::decode_block's output, DC
// predicted) of an in-scope frame, in scan order, with the Cr blocks zeroed as
// the device never stores them.  Returns the number of blocks, or -1.
JH_API int64_t jh_host_coefficients(const uint8_t* data, size_t size, int16_t* coef_out, int64_t coef_cap) {
  lmj::Header h;
  lmj::parse(data, size, h);
  if (h.cls != lmj::kInScope) return -1;
  std::vector<int16_t> coef;
  if (!locomouse::decode_jpeg_coefficients(data, size, coef)) return -1;
  const LmjScan sc = lmj::make_scan(h, 64);
  if (coef.size() != (size_t)sc.nblk * 64 || (int64_t)coef.size() > coef_cap) return -1;
  for (uint32_t blk = 0; blk < sc.nblk; ++blk)
    if (lmj_comp_of(sc, blk % sc.bpm) >= 2) std::memset(coef.data() + (size_t)blk * 64, 0, 128);
  std::memcpy(coef_out, coef.data(), coef.size() * sizeof(int16_t));
  return (int64_t)sc.nblk;
}
