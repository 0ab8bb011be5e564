// Jpeg.cpp — sequential Huffman JPEG decoding to BGR channel 0 (see Jpeg.hpp).
//
// The stream is decoded component plane by component plane (every block's
// coefficients straight through the ISLOW IDCT into its plane; a plane not
// needed for channel 0 — Cr of a YCbCr image — is entropy-decoded only), then
// channel 0 is formed row by row from the planes.  The arithmetic follows
// ITU-T T.81 (Huffman decoding F.2.2, restart markers B.2.1) and libjpeg's
// decompression defaults (jidctint.c, jdsample.c, jdcolor.c), the decoder
// the reference's OpenCV build links for still images.
#include "Jpeg.hpp"

#include "../csrc/lm_jpeg_hdr.h"

#include <algorithm>
#include <cstring>

namespace locomouse {
namespace {

// Header parsing, the Huffman tables and the zig-zag order are shared with the
// device decoder (csrc/lm_jpeg_hdr.h).
using lmj::kNatural;
using Huff = lmj::HuffTable;
constexpr int kLook = LMJ_LOOK;  // Huffman lookahead bits

// Entropy-coded segment reader: byte stuffing (FF 00) removed, fill bytes
// (FF FF ..) skipped, stops at a marker and feeds zeros past it (libjpeg's
// behaviour on premature markers).
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf = 0;
  int cnt = 0;
  bool marker = false;

  void refill() {
    while (cnt <= 56) {
      unsigned b = 0;
      if (!marker && p < end) {
        b = *p++;
        if (b == 0xFF) {
          const uint8_t* q = p;
          while (q < end && *q == 0xFF) ++q;
          if (q < end && *q == 0) {
            p = q + 1;
          } else {  // a marker: leave p on its FF
            marker = true;
            p = q - 1;
            b = 0;
          }
        }
      }
      buf |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  unsigned get(int n) {  // n in 1..16, cnt >= n
    const unsigned v = (unsigned)(buf >> (64 - n));
    buf <<= n;
    cnt -= n;
    return v;
  }
  int decode(const Huff& h) {
    const unsigned e = h.look[buf >> (64 - kLook)];
    if (e >> 8) {
      buf <<= (e >> 8);
      cnt -= (int)(e >> 8);
      return (int)(e & 255);
    }
    int l = kLook + 1;
    int32_t code = (int32_t)(buf >> (64 - l));
    while (code > h.maxcode[l]) {
      ++l;
      code = (int32_t)(buf >> (64 - l));
    }
    if (l > 16) {  // not a code (corrupt data): libjpeg returns symbol 0
      buf <<= 16;
      cnt -= 16;
      return 0;
    }
    buf <<= l;
    cnt -= l;
    return h.vals[(code + h.valoff[l]) & 255];
  }
  // Restart: drop the remaining bits, step over the RSTn marker.
  void restart() {
    buf = 0;
    cnt = 0;
    if (!marker) {  // find the marker
      while (p < end) {
        if (*p == 0xFF && p + 1 < end && p[1] != 0 && p[1] != 0xFF) break;
        ++p;
      }
    }
    if (p + 1 < end && p[1] >= 0xD0 && p[1] <= 0xD7) p += 2;
    marker = false;
  }
};

inline int extend(unsigned v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// libjpeg's post-IDCT range limit: x + 128 clamped to 0..255 for |x| < 512,
// wrapping by 1024 beyond (prepare_range_limit_table's layout).
struct RangeLimit {
  uint8_t t[1024];
  RangeLimit() {
    for (int i = 0; i < 1024; ++i) {
      if (i < 128) t[i] = (uint8_t)(i + 128);
      else if (i < 512) t[i] = 255;
      else if (i < 896) t[i] = 0;
      else t[i] = (uint8_t)(i - 896);
    }
  }
};
const RangeLimit kRange;

// ISLOW inverse DCT (libjpeg jidctint.c: Loeffler-Ligtenberg-Moschytz with
// 13-bit constants, 2 extra bits between the column and row passes), with
// dequantisation folded into the column pass.
constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633,
                  F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
constexpr int kConstBits = 13, kPass1 = 2;

// JLONG arithmetic (64-bit on LP64, as jidctint.c): with 16-bit quantisation
// tables (SOF1) the products exceed 32 bits.  The column pass's workspace is
// int, as libjpeg's.
inline int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }
inline int64_t left_shift(int64_t a, int b) { return (int64_t)((uint64_t)a << b); }  // LEFT_SHIFT (jdct.h)

void idct_islow(const int16_t* coef, const uint16_t* q, uint8_t* out, int pitch) {
  int32_t ws[64];
  for (int c = 0; c < 8; ++c) {
    const int16_t* in = coef + c;
    const uint16_t* qq = q + c;
    int32_t* w = ws + c;
    if (!(in[8] | in[16] | in[24] | in[32] | in[40] | in[48] | in[56])) {
      const int32_t dc = (int32_t)left_shift((int32_t)in[0] * (int32_t)qq[0], kPass1);  // int dcval (wraps like libjpeg)
      for (int r = 0; r < 8; ++r) w[8 * r] = dc;
      continue;
    }
    int64_t z2 = (int32_t)in[16] * (int32_t)qq[16], z3 = (int32_t)in[48] * (int32_t)qq[48];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
    z2 = (int32_t)in[0] * (int32_t)qq[0];
    z3 = (int32_t)in[32] * (int32_t)qq[32];
    int64_t tmp0 = left_shift(z2 + z3, kConstBits), tmp1 = left_shift(z2 - z3, kConstBits);
    const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    tmp0 = (int32_t)in[56] * (int32_t)qq[56];
    tmp1 = (int32_t)in[40] * (int32_t)qq[40];
    tmp2 = (int32_t)in[24] * (int32_t)qq[24];
    tmp3 = (int32_t)in[8] * (int32_t)qq[8];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * F1175;
    tmp0 *= F0298;
    tmp1 *= F2053;
    tmp2 *= F3072;
    tmp3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int s = kConstBits - kPass1;
    w[0] = (int32_t)descale(t10 + tmp3, s);
    w[56] = (int32_t)descale(t10 - tmp3, s);
    w[8] = (int32_t)descale(t11 + tmp2, s);
    w[48] = (int32_t)descale(t11 - tmp2, s);
    w[16] = (int32_t)descale(t12 + tmp1, s);
    w[40] = (int32_t)descale(t12 - tmp1, s);
    w[24] = (int32_t)descale(t13 + tmp0, s);
    w[32] = (int32_t)descale(t13 - tmp0, s);
  }
  constexpr int s2 = kConstBits + kPass1 + 3;
  for (int r = 0; r < 8; ++r) {
    const int32_t* w = ws + 8 * r;
    uint8_t* o = out + (size_t)r * pitch;
    if (!(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7])) {
      const uint8_t v = kRange.t[(int)descale(w[0], kPass1 + 3) & 1023];
      std::memset(o, v, 8);
      continue;
    }
    int64_t z2 = w[2], z3 = w[6];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
    int64_t tmp0 = left_shift((int64_t)w[0] + w[4], kConstBits), tmp1 = left_shift((int64_t)w[0] - w[4], kConstBits);
    const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    tmp0 = w[7];
    tmp1 = w[5];
    tmp2 = w[3];
    tmp3 = w[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * F1175;
    tmp0 *= F0298;
    tmp1 *= F2053;
    tmp2 *= F3072;
    tmp3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = kRange.t[(int)descale(t10 + tmp3, s2) & 1023];
    o[7] = kRange.t[(int)descale(t10 - tmp3, s2) & 1023];
    o[1] = kRange.t[(int)descale(t11 + tmp2, s2) & 1023];
    o[6] = kRange.t[(int)descale(t11 - tmp2, s2) & 1023];
    o[2] = kRange.t[(int)descale(t12 + tmp1, s2) & 1023];
    o[5] = kRange.t[(int)descale(t12 - tmp1, s2) & 1023];
    o[3] = kRange.t[(int)descale(t13 + tmp0, s2) & 1023];
    o[4] = kRange.t[(int)descale(t13 - tmp0, s2) & 1023];
  }
}

// jdcolor.c's Cb -> B term: round(1.772 * 2^16 * (cb - 128)) >> 16.
struct CbToB {
  int16_t t[256];
  CbToB() {
    const int32_t fix = (int32_t)(1.772 * 65536.0 + 0.5);
    for (int i = 0; i < 256; ++i) t[i] = (int16_t)((fix * (i - 128) + (1 << 15)) >> 16);
  }
};
const CbToB kCbB;

struct Component : lmj::CompBase {
  int pred = 0;
  bool need = false;       // plane feeds channel 0
  std::vector<uint8_t> plane;
};

// The segment walk and its state are lmj::HeaderState's; this adds the scans.
struct Decoder : lmj::HeaderState<Component> {
  std::vector<int16_t>* coef_sink = nullptr;  // tests: every block's coefficients, in decoding order

  void decode_block(Bits& b, Component& C, int16_t* blk) {
    std::memset(blk, 0, 64 * sizeof(int16_t));
    if (b.cnt < 32) b.refill();
    const int s = b.decode(dc[C.td]);
    if (s) {
      if (b.cnt < 16) b.refill();
      C.pred += extend(b.get(s > 16 ? 16 : s), s > 16 ? 16 : s);
    }
    blk[0] = (int16_t)C.pred;
    const Huff& A = ac[C.ta];
    for (int k = 1; k < 64;) {
      if (b.cnt < 32) b.refill();
      const int rs = b.decode(A);
      const int r = rs >> 4, sz = rs & 15;
      if (sz) {
        k += r;
        blk[kNatural[k]] = (int16_t)extend(b.get(sz), sz);
        ++k;
      } else {
        if (r != 15) break;
        k += 16;
      }
    }
  }

  // One scan (interleaved when ns > 1), starting at `data`; returns the
  // position after the entropy-coded segment (at its terminating marker).
  const uint8_t* decode_scan(const uint8_t* data, const uint8_t* end, int ns, const int* idx) {
    Bits b{data, end};
    for (int i = 0; i < ns; ++i) comp[idx[i]].pred = 0;
    int16_t blk[64];
    const bool single = ns == 1;
    const int mcux = single ? (comp[idx[0]].dw + 7) / 8 : (W + 8 * hmax - 1) / (8 * hmax);
    const int mcuy = single ? (comp[idx[0]].dh + 7) / 8 : (H + 8 * vmax - 1) / (8 * vmax);
    int todo = restart;
    for (int my = 0; my < mcuy; ++my)
      for (int mx = 0; mx < mcux; ++mx) {
        if (restart && todo == 0) {
          b.restart();
          for (int i = 0; i < ns; ++i) comp[idx[i]].pred = 0;
          todo = restart;
        }
        for (int i = 0; i < ns; ++i) {
          Component& C = comp[idx[i]];
          const int bh = single ? 1 : C.h, bv = single ? 1 : C.v;
          for (int v = 0; v < bv; ++v)
            for (int h = 0; h < bh; ++h) {
              decode_block(b, C, blk);
              if (coef_sink) coef_sink->insert(coef_sink->end(), blk, blk + 64);
              if (!C.need) continue;
              const int bx = mx * bh + h, by = my * bv + v;
              idct_islow(blk, qt[C.tq], C.plane.data() + (size_t)by * 8 * C.pitch + bx * 8, C.pitch);
            }
        }
        --todo;
      }
    // Leave the reader on the next marker.
    const uint8_t* p = b.p;
    if (!b.marker)
      while (p + 1 < end && !(p[0] == 0xFF && p[1] != 0 && p[1] != 0xFF)) ++p;
    return p;
  }

  bool run(const uint8_t* d, size_t n) {
    return walk(d, n, [this](const uint8_t* p, const uint8_t* end, int ns, const int* idx, bool first) {
      if (first) {  // first scan: decide which planes channel 0 needs
        for (int c = 0; c < nc; ++c) {
          comp[c].need = needed(c);
          if (comp[c].need) comp[c].plane.assign((size_t)comp[c].pitch * comp[c].prows, 0);
        }
      }
      fill_default_tables();
      for (int i = 0; i < ns; ++i) {
        const Component& C = comp[idx[i]];
        if (!dc[C.td].defined || !ac[C.ta].defined) {
          fail("scan uses an undefined Huffman table");
          return (const uint8_t*)nullptr;
        }
        if (C.need && !qdef[C.tq]) {
          fail("component uses an undefined quantisation table");
          return (const uint8_t*)nullptr;
        }
      }
      return decode_scan(p, end, ns, idx);
    });
  }

  // Plane row y of component C at full resolution (upsampled by libjpeg's
  // fancy filters for 2x horizontal and/or 2x vertical, by replication for
  // other ratios) into `o` (W samples).
  void upsample_row(const Component& C, int y, uint8_t* o, std::vector<int>& tmp) const {
    const int hx = hmax / C.h, vx = vmax / C.v;
    const bool hfit = hmax % C.h == 0, vfit = vmax % C.v == 0;
    const uint8_t* P = C.plane.data();
    if (hx == 1 && vx == 1 && hfit && vfit) {
      std::memcpy(o, P + (size_t)y * C.pitch, (size_t)W);
      return;
    }
    if ((hx == 2 || hx == 1) && (vx == 2 || vx == 1) && hfit && vfit) {
      const int dw = C.dw;
      if (vx == 2) {  // vertical triangle: 3/4 nearer row + 1/4 the next one (edge rows replicate)
        const int r = y >> 1;
        const int r2 = (y & 1) ? std::min(r + 1, C.dh - 1) : std::max(r - 1, 0);
        const uint8_t* a = P + (size_t)r * C.pitch;
        const uint8_t* b = P + (size_t)r2 * C.pitch;
        tmp.resize((size_t)dw);
        for (int x = 0; x < dw; ++x) tmp[x] = 3 * a[x] + b[x];
        if (hx == 1) {  // h1v2_fancy_upsample
          const int bias = (y & 1) ? 2 : 1;
          for (int x = 0; x < W; ++x) o[x] = (uint8_t)((tmp[x] + bias) >> 2);
          return;
        }
        // h2v2_fancy_upsample
        auto put = [&](int ox, int v) {
          if (ox < W) o[ox] = (uint8_t)v;
        };
        if (dw == 1) {
          put(0, (tmp[0] * 4 + 8) >> 4);
          put(1, (tmp[0] * 4 + 7) >> 4);
          return;
        }
        put(0, (tmp[0] * 4 + 8) >> 4);
        put(1, (tmp[0] * 3 + tmp[1] + 7) >> 4);
        for (int x = 1; x < dw - 1; ++x) {
          put(2 * x, (tmp[x] * 3 + tmp[x - 1] + 8) >> 4);
          put(2 * x + 1, (tmp[x] * 3 + tmp[x + 1] + 7) >> 4);
        }
        put(2 * dw - 2, (tmp[dw - 1] * 3 + tmp[dw - 2] + 8) >> 4);
        put(2 * dw - 1, (tmp[dw - 1] * 4 + 7) >> 4);
        return;
      }
      // h2v1_fancy_upsample
      const uint8_t* a = P + (size_t)y * C.pitch;
      auto put = [&](int ox, int v) {
        if (ox < W) o[ox] = (uint8_t)v;
      };
      if (dw == 1) {
        put(0, a[0]);
        put(1, a[0]);
        return;
      }
      put(0, a[0]);
      put(1, (a[0] * 3 + a[1] + 2) >> 2);
      for (int x = 1; x < dw - 1; ++x) {
        put(2 * x, (a[x] * 3 + a[x - 1] + 1) >> 2);
        put(2 * x + 1, (a[x] * 3 + a[x + 1] + 2) >> 2);
      }
      put(2 * dw - 2, (a[dw - 1] * 3 + a[dw - 2] + 1) >> 2);
      put(2 * dw - 1, a[dw - 1]);
      return;
    }
    // Integral (or non-integral) ratios: sample replication.
    const int r = std::min(y * C.v / vmax, C.prows - 1);
    const uint8_t* a = P + (size_t)r * C.pitch;
    for (int x = 0; x < W; ++x) o[x] = a[std::min(x * C.h / hmax, C.pitch - 1)];
  }

  void channel0(uint8_t* out) const {
    std::vector<int> tmp;
    if (nc == 1) {
      for (int y = 0; y < H; ++y) upsample_row(comp[0], y, out + (size_t)y * W, tmp);
      return;
    }
    if (is_rgb()) {  // channel 0 = B = third component
      for (int y = 0; y < H; ++y) upsample_row(comp[2], y, out + (size_t)y * W, tmp);
      return;
    }
    std::vector<uint8_t> cb((size_t)W);
    for (int y = 0; y < H; ++y) {
      uint8_t* o = out + (size_t)y * W;
      upsample_row(comp[0], y, o, tmp);
      upsample_row(comp[1], y, cb.data(), tmp);
      for (int x = 0; x < W; ++x) {
        const int b = o[x] + kCbB.t[cb[x]];
        o[x] = (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
      }
    }
  }
};

}  // namespace

bool decode_jpeg_channel0(const uint8_t* data, size_t size, int& rows, int& cols, std::vector<uint8_t>& out,
                          std::string* err) {
  Decoder D;
  if (!D.run(data, size)) {
    if (err) *err = D.why;
    return false;
  }
  rows = D.H;
  cols = D.W;
  out.resize((size_t)rows * cols);
  D.channel0(out.data());
  return true;
}

bool decode_jpeg_coefficients(const uint8_t* data, size_t size, std::vector<int16_t>& coef, std::string* err) {
  Decoder D;
  coef.clear();
  D.coef_sink = &coef;
  if (!D.run(data, size)) {
    if (err) *err = D.why;
    return false;
  }
  return true;
}

bool decode_jpeg_channel0_into(const uint8_t* data, size_t size, int rows, int cols, uint8_t* out, std::string* err) {
  Decoder D;
  if (!D.run(data, size)) {
    if (err) *err = D.why;
    return false;
  }
  if (D.H != rows || D.W != cols) {
    if (err)
      *err = "JPEG frame is " + std::to_string(D.W) + "x" + std::to_string(D.H) + ", the video header says " +
             std::to_string(cols) + "x" + std::to_string(rows);
    return false;
  }
  D.channel0(out);
  return true;
}

}  // namespace locomouse
