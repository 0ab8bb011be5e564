// JpegEncode.cpp — see JpegEncode.hpp.  The blocks' coefficients come from
// csrc/lm_jpeg_enc_core.h (shared with the kernels); the entropy coder below is
// jchuff.c's encode_one_block with its byte stuffing.
#include "JpegEncode.hpp"

#include "../csrc/lm_jpeg_enc_core.h"

#include <stdexcept>

namespace locomouse {

namespace {

struct BitWriter {
  std::vector<uint8_t>& out;
  uint32_t acc = 0;
  int n = 0;
  void put(uint32_t code, int len) {  // len <= 16
    acc = (acc << len) | (code & ((1u << len) - 1));
    n += len;
    while (n >= 8) {
      const uint8_t b = (uint8_t)(acc >> (n - 8));
      out.push_back(b);
      if (b == 0xFF) out.push_back(0);
      n -= 8;
    }
  }
  void flush() {  // the last partial byte is filled with 1-bits (and stuffed like any other)
    if (n) put(0x7F, 8 - n);
  }
};

void check(const uint8_t* pixels, int rows, int cols, int quality) {
  if (!pixels) throw std::invalid_argument("encode_jpeg: pixels is NULL");
  if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535) throw std::invalid_argument("encode_jpeg: rows and cols must be in 1..65535");
  if (quality < 1 || quality > 100) throw std::invalid_argument("encode_jpeg: quality must be in 1..100");
}

}  // namespace

void encode_jpeg_coefficients(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality,
                              std::vector<int16_t>& coef) {
  check(pixels, rows, cols, quality);
  const LjeGeom g = lje_geom(rows, cols, (int)format);
  LjeTables T;
  lje::make_tables(quality, T);
  coef.assign((size_t)g.nblk * 64, 0);
  for (uint32_t b = 0; b < g.nblk; ++b) lje::block_coefficients(pixels, g, T, b, coef.data() + (size_t)b * 64);
}

void encode_jpeg(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality, std::vector<uint8_t>& out,
                 int restart_interval) {
  check(pixels, rows, cols, quality);
  if (restart_interval < 0 || restart_interval > 65535) throw std::invalid_argument("encode_jpeg: restart_interval must be in 0..65535");
  const LjeGeom g = lje_geom(rows, cols, (int)format);
  LjeTables T;
  lje::make_tables(quality, T);
  const std::vector<uint8_t> h = lje::header(rows, cols, (int)format, quality, restart_interval);
  out.insert(out.end(), h.begin(), h.end());
  BitWriter w{out};
  int last_dc[3] = {0, 0, 0};
  int16_t c[64];
  const uint32_t bpi = (uint32_t)restart_interval * (uint32_t)g.bpm;  // blocks of an interval
  uint32_t marker = 0;
  for (uint32_t b = 0; b < g.nblk; ++b) {
    if (bpi && b && b % bpi == 0) {  // jchuff.c emit_restart
      w.flush();
      out.push_back(0xFF);
      out.push_back((uint8_t)(0xD0 + (marker++ & 7)));
      last_dc[0] = last_dc[1] = last_dc[2] = 0;
    }
    lje::block_coefficients(pixels, g, T, b, c);
    const int comp = lje_block(g, b).comp;
    const uint32_t* e = T.ehuf + (comp ? LJE_EHUF_STRIDE : 0);
    const int diff = c[0] - last_dc[comp];
    last_dc[comp] = c[0];
    int nb = lje_cat_dc(lje_nbits(diff));
    w.put(e[nb] >> 5, (int)(e[nb] & 31));
    if (nb) w.put((uint32_t)(diff < 0 ? diff - 1 : diff), nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
      const int v = c[k];
      if (!v) {
        ++run;
        continue;
      }
      for (; run > 15; run -= 16) w.put(e[16 + 0xF0] >> 5, (int)(e[16 + 0xF0] & 31));
      nb = lje_cat_ac(lje_nbits(v));
      const uint32_t s = e[16 + (run << 4 | nb)];
      w.put(s >> 5, (int)(s & 31));
      w.put((uint32_t)(v < 0 ? v - 1 : v), nb);
      run = 0;
    }
    if (run) w.put(e[16] >> 5, (int)(e[16] & 31));
  }
  w.flush();
  out.push_back(0xFF);
  out.push_back(0xD9);
}

}  // namespace locomouse
