// lm_jpeg_enc_core.h — the baseline JPEG encoder's arithmetic
// (include/locomouse_encode.h), compiled for host and device: the block
// geometry of a scan, the sample fetch with libjpeg's edge rules, RGB -> YCbCr,
// h2v2 downsampling, the ISLOW forward DCT, quantisation and the size category
// of a coefficient.  The host encoder (host/JpegEncode.cpp) and the kernels
// (lm_jpeg_enc.hip) both run these functions, so their integers are the same
// by construction.  Integers only.
//
// Everything restates libjpeg's defaults (jcparam.c, jccolor.c, jcsample.c,
// jcprepct.c, jccoefct.c, jfdctint.c, jcdctmgr.c, jchuff.c), pinned through
// Pillow byte for byte (tests/test_jpeg_encode.py).
#ifndef LM_JPEG_ENC_CORE_H
#define LM_JPEG_ENC_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LJE_HD __host__ __device__ inline
#else
#define LJE_HD inline
#endif

#define LJE_GRAY8 0  // one component; a frame is rows x cols u8
#define LJE_RGB24 1  // YCbCr 4:2:0; a frame is rows x cols x 3 u8 (R, G, B)

// Worst case of one block's entropy-coded bits with the Annex K tables, the
// size categories clamped as lje_cat_dc / lje_cat_ac clamp them:
//   DC: the longest DC code is 11 bits (chroma, category 11) and a value field
//       is at most 11 bits: 22;
//   AC: every code is at most 16 bits and a value field at most 10: 26 for a
//       non-zero coefficient.  A ZRL (<= 16 bits) stands for 16 zero
//       coefficients and an EOB (<= 16 bits) for at least one, so neither
//       costs more than the 26 bits per coefficient they replace.
//   22 + 63 * 26 = 1660 bits, rounded up to whole 32-bit words: 52 words.
#define LJE_BLOCK_BITS 1660
#define LJE_BLOCK_WORDS 52
static_assert(LJE_BLOCK_WORDS * 32 >= LJE_BLOCK_BITS, "a block's worst case fits its words");
#define LJE_MAX_HEADER 640  // SOI .. SOS of the colour layout is 623 bytes, 629 with a DRI segment (lje::header checks it)

struct LjeGeom {
  int32_t rows, cols, format;
  int32_t bw, bh;  // component 0 in blocks: ceil(cols / 8), ceil(rows / 8)
  int32_t mw, mh;  // MCUs: 8 x 8 (grey) or 16 x 16 (colour)
  int32_t cw, ch;  // downsampled chroma size: ceil(cols / 2), ceil(rows / 2)
  int32_t bpm;     // blocks per MCU: 1 or 6 (Y00 Y01 Y10 Y11 Cb Cr)
  uint32_t nblk;   // blocks of the scan
};

LJE_HD LjeGeom lje_geom(int32_t rows, int32_t cols, int32_t format) {
  LjeGeom g;
  g.rows = rows;
  g.cols = cols;
  g.format = format;
  g.bw = (cols + 7) / 8;
  g.bh = (rows + 7) / 8;
  g.cw = (cols + 1) / 2;
  g.ch = (rows + 1) / 2;
  if (format == LJE_RGB24) {
    g.mw = (cols + 15) / 16;
    g.mh = (rows + 15) / 16;
    g.bpm = 6;
  } else {
    g.mw = g.bw;
    g.mh = g.bh;
    g.bpm = 1;
  }
  g.nblk = (uint32_t)g.mw * (uint32_t)g.mh * (uint32_t)g.bpm;
  return g;
}

// Block b of the scan: its component, the block of that component whose
// samples it transforms, and whether it is a dummy block (jccoefct.c): all AC
// zero and the DC of block (br, bc), the block libjpeg copies the DC from.
struct LjeBlock {
  int32_t comp;  // 0 Y, 1 Cb, 2 Cr
  int32_t br, bc;
  int32_t dummy;
};

LJE_HD LjeBlock lje_block(const LjeGeom& g, uint32_t b) {
  LjeBlock k;
  k.dummy = 0;
  if (g.bpm == 1) {
    k.comp = 0;
    k.br = (int32_t)(b / (uint32_t)g.mw);
    k.bc = (int32_t)(b % (uint32_t)g.mw);
    return k;
  }
  const uint32_t m = b / 6u;
  const int32_t j = (int32_t)(b % 6u);
  const int32_t my = (int32_t)(m / (uint32_t)g.mw), mx = (int32_t)(m % (uint32_t)g.mw);
  if (j >= 4) {
    k.comp = j - 3;
    k.br = my;
    k.bc = mx;
    return k;
  }
  k.comp = 0;
  k.br = 2 * my + (j >> 1);
  k.bc = 2 * mx + (j & 1);
  if (k.br >= g.bh) {  // a dummy row: the DC of the block in front of it in the MCU
    k.dummy = 1;
    k.br = 2 * my;
    k.bc = 2 * mx + 1 < g.bw ? 2 * mx + 1 : 2 * mx;
  } else if (k.bc >= g.bw) {  // a dummy block at the right edge: the DC of its left neighbour
    k.dummy = 1;
    k.bc = 2 * mx;
  }
  return k;
}

// The block in front of block b in its component's DC prediction, or -1.
LJE_HD int64_t lje_dc_pred_block(const LjeGeom& g, uint32_t b) {
  if (g.bpm == 1) return (int64_t)b - 1;
  const uint32_t j = b % 6u;
  if (j >= 1 && j <= 3) return (int64_t)b - 1;
  if (b < 6u) return -1;
  return j == 0 ? (int64_t)b - 3 : (int64_t)b - 6;  // Y3 of the MCU before; its Cb / Cr
}

// The same with a restart interval of ri > 0 MCUs (jchuff.c emit_restart): the
// first MCU of an interval predicts every component from 0.
LJE_HD int64_t lje_dc_pred_block_rst(const LjeGeom& g, uint32_t b, uint32_t ri) {
  const uint32_t j = b % (uint32_t)g.bpm;
  if (j >= 1 && j <= 3) return (int64_t)b - 1;
  return (b / (uint32_t)g.bpm) % ri == 0 ? -1 : lje_dc_pred_block(g, b);
}

// Restart intervals of a scan of `ri` MCUs each (ri > 0): ceil(MCUs / ri).  All
// but the last end in a marker.
LJE_HD uint32_t lje_intervals(const LjeGeom& g, uint32_t ri) {
  const uint32_t nmcu = g.nblk / (uint32_t)g.bpm;
  return (nmcu + ri - 1) / ri;
}

// jccolor.c rgb_ycc_convert, 16 fractional bits.
LJE_HD int32_t lje_y(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
LJE_HD int32_t lje_cb(int32_t r, int32_t g, int32_t b) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
LJE_HD int32_t lje_cr(int32_t r, int32_t g, int32_t b) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Sample (r, c) of the padded component 0: rows and columns past the image
// repeat its last row / column.
LJE_HD int32_t lje_sample_y(const uint8_t* f, const LjeGeom& g, int32_t r, int32_t c) {
  r = r < g.rows ? r : g.rows - 1;
  c = c < g.cols ? c : g.cols - 1;
  if (g.format == LJE_GRAY8) return f[(size_t)r * (size_t)g.cols + (size_t)c];
  const uint8_t* p = f + ((size_t)r * (size_t)g.cols + (size_t)c) * 3;
  return lje_y(p[0], p[1], p[2]);
}

// Sample (r, c) of the padded, downsampled chroma component (1 Cb, 2 Cr):
// the input rows are extended to an even count and the columns to the right by
// repetition, four converted pixels are averaged with the bias 1, 2, 1, 2 ...
// along the output row (jcsample.c h2v2_downsample), and rows below the last
// downsampled one repeat it.
LJE_HD int32_t lje_sample_c(const uint8_t* f, const LjeGeom& g, int32_t comp, int32_t r, int32_t c) {
  r = r < g.ch ? r : g.ch - 1;
  const int32_t r0 = 2 * r, r1 = 2 * r + 1 < g.rows ? 2 * r + 1 : g.rows - 1;
  const int32_t c0 = 2 * c < g.cols ? 2 * c : g.cols - 1, c1 = 2 * c + 1 < g.cols ? 2 * c + 1 : g.cols - 1;
  int32_t sum = (c & 1) ? 2 : 1;
  const uint8_t* p00 = f + ((size_t)r0 * (size_t)g.cols + (size_t)c0) * 3;
  const uint8_t* p01 = f + ((size_t)r0 * (size_t)g.cols + (size_t)c1) * 3;
  const uint8_t* p10 = f + ((size_t)r1 * (size_t)g.cols + (size_t)c0) * 3;
  const uint8_t* p11 = f + ((size_t)r1 * (size_t)g.cols + (size_t)c1) * 3;
  if (comp == 1)
    sum += lje_cb(p00[0], p00[1], p00[2]) + lje_cb(p01[0], p01[1], p01[2]) + lje_cb(p10[0], p10[1], p10[2]) +
           lje_cb(p11[0], p11[1], p11[2]);
  else
    sum += lje_cr(p00[0], p00[1], p00[2]) + lje_cr(p01[0], p01[1], p01[2]) + lje_cr(p10[0], p10[1], p10[2]) +
           lje_cr(p11[0], p11[1], p11[2]);
  return sum >> 2;
}

// Sample (r, c) of a block's component, level-shifted.
LJE_HD int32_t lje_sample(const uint8_t* f, const LjeGeom& g, int32_t comp, int32_t r, int32_t c) {
  return (comp == 0 ? lje_sample_y(f, g, r, c) : lje_sample_c(f, g, comp, r, c)) - 128;
}

// jfdctint.c, CONST_BITS 13, PASS1_BITS 2: one 8-point pass over d[0..8).
// pass 1 works on a row of samples, pass 2 on a column of pass-1 results; the
// results are 8 times the DCT.  (d is indexed with constants only.)
#define LJE_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))
template <int PASS>
LJE_HD void lje_fdct8(int32_t* d) {
  const int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
  const int32_t tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
  const int32_t tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
  const int32_t tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int S = PASS == 1 ? 13 - 2 : 13 + 2;
  if (PASS == 1) {
    d[0] = (tmp10 + tmp11) * 4;
    d[4] = (tmp10 - tmp11) * 4;
  } else {
    d[0] = LJE_DESCALE(tmp10 + tmp11, 2);
    d[4] = LJE_DESCALE(tmp10 - tmp11, 2);
  }
  int32_t z1 = (tmp12 + tmp13) * 4433;
  d[2] = LJE_DESCALE(z1 + tmp13 * 6270, S);
  d[6] = LJE_DESCALE(z1 + tmp12 * (-15137), S);
  z1 = tmp4 + tmp7;
  int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int32_t z5 = (z3 + z4) * 9633;
  const int32_t t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  d[7] = LJE_DESCALE(t4 + z1 + z3, S);
  d[5] = LJE_DESCALE(t5 + z2 + z4, S);
  d[3] = LJE_DESCALE(t6 + z2 + z3, S);
  d[1] = LJE_DESCALE(t7 + z1 + z4, S);
}

// jcdctmgr.c: v is 8 times the coefficient, div is 8 * the table entry.
LJE_HD int32_t lje_quant(int32_t v, int32_t div) {
  return v < 0 ? -((-v + (div >> 1)) / div) : (v + (div >> 1)) / div;
}

// Bits of |v|.
LJE_HD int32_t lje_nbits(int32_t v) {
  uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int32_t n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  return n;
}
// The size category of a DC difference / an AC coefficient.  The arithmetic
// above keeps them within 11 / 10 bits for 8-bit samples; the clamp makes the
// bound of LJE_BLOCK_BITS hold whatever a coefficient buffer contains.
LJE_HD int32_t lje_cat_dc(int32_t n) { return n > 11 ? 11 : n; }
LJE_HD int32_t lje_cat_ac(int32_t n) { return n > 10 ? 10 : n; }

// The encoder's Huffman tables as the coders index them: table t (0 luma, 1
// chroma), entry s: 0..15 the DC category s, 16 + s the AC symbol s (run << 4 |
// category).  An entry is code << 5 | length; length 0 marks a symbol the
// Annex K tables lack (none that the coders produce).
#define LJE_EHUF_STRIDE 272
struct LjeTables {
  uint16_t div[2][64];                 // 8 * quantisation table, natural order
  uint32_t ehuf[2 * LJE_EHUF_STRIDE];  // code << 5 | length
  uint8_t pos[64];                     // natural index -> zig-zag position
};

// ------------------------------------------------------------------ host only
#include <vector>

#include "lm_jpeg_hdr.h"

namespace lje {

constexpr uint8_t kLumQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jcparam.c jpeg_set_quality with force_baseline: table t at `quality` (1..100), natural order.
inline void quant_table(int quality, int t, uint8_t out[64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const uint8_t* base = t ? kChromQ : kLumQ;
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * scale + 50) / 100;
    out[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

inline void fill_ehuf(uint32_t* e, int first, const uint8_t bits[16], const uint8_t* vals) {
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) e[first + vals[k]] = code << 5 | (uint32_t)l;
    code <<= 1;
  }
}

inline void make_tables(int quality, LjeTables& T) {
  for (int t = 0; t < 2; ++t) {
    uint8_t q[64];
    quant_table(quality, t, q);
    for (int i = 0; i < 64; ++i) T.div[t][i] = (uint16_t)(8 * q[i]);
  }
  for (uint32_t& e : T.ehuf) e = 0;
  fill_ehuf(T.ehuf, 0, lmj::kDcLumBits, lmj::kDcVals);
  fill_ehuf(T.ehuf, 16, lmj::kAcLumBits, lmj::kAcLumVals);
  fill_ehuf(T.ehuf, LJE_EHUF_STRIDE, lmj::kDcChromBits, lmj::kDcVals);
  fill_ehuf(T.ehuf, LJE_EHUF_STRIDE + 16, lmj::kAcChromBits, lmj::kAcChromVals);
  for (int k = 0; k < 64; ++k) T.pos[lmj::kNatural[k]] = (uint8_t)k;
}

// SOI .. SOS as libjpeg writes them for these settings (jcmarker.c).  A
// restart interval > 0 (in MCUs, at most 65535) adds the DRI segment where
// write_scan_header puts it: behind the DHT segments, in front of SOS.
inline std::vector<uint8_t> header(int rows, int cols, int format, int quality, int restart_interval = 0) {
  std::vector<uint8_t> h = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  const int nc = format == LJE_RGB24 ? 3 : 1, nt = nc == 3 ? 2 : 1;
  for (int t = 0; t < nt; ++t) {
    uint8_t q[64];
    quant_table(quality, t, q);
    h.insert(h.end(), {0xFF, 0xDB, 0, 67, (uint8_t)t});
    for (int k = 0; k < 64; ++k) h.push_back(q[lmj::kNatural[k]]);
  }
  h.insert(h.end(), {0xFF, 0xC0, 0, (uint8_t)(8 + 3 * nc), 8, (uint8_t)(rows >> 8), (uint8_t)rows, (uint8_t)(cols >> 8),
                     (uint8_t)cols, (uint8_t)nc});
  for (int c = 0; c < nc; ++c) h.insert(h.end(), {(uint8_t)(c + 1), (uint8_t)(nc == 3 && c == 0 ? 0x22 : 0x11), (uint8_t)(c ? 1 : 0)});
  const struct {
    uint8_t id;
    const uint8_t* bits;
    const uint8_t* vals;
  } dht[4] = {{0x00, lmj::kDcLumBits, lmj::kDcVals},
              {0x10, lmj::kAcLumBits, lmj::kAcLumVals},
              {0x01, lmj::kDcChromBits, lmj::kDcVals},
              {0x11, lmj::kAcChromBits, lmj::kAcChromVals}};
  for (int t = 0; t < 2 * nt; ++t) {
    int n = 0;
    for (int l = 0; l < 16; ++l) n += dht[t].bits[l];
    h.insert(h.end(), {0xFF, 0xC4, (uint8_t)((19 + n) >> 8), (uint8_t)(19 + n), dht[t].id});
    h.insert(h.end(), dht[t].bits, dht[t].bits + 16);
    h.insert(h.end(), dht[t].vals, dht[t].vals + n);
  }
  if (restart_interval > 0) h.insert(h.end(), {0xFF, 0xDD, 0, 4, (uint8_t)(restart_interval >> 8), (uint8_t)restart_interval});
  h.insert(h.end(), {0xFF, 0xDA, 0, (uint8_t)(6 + 2 * nc), (uint8_t)nc});
  for (int c = 0; c < nc; ++c) h.insert(h.end(), {(uint8_t)(c + 1), (uint8_t)(c ? 0x11 : 0x00)});
  h.insert(h.end(), {0, 63, 0});
  return h;
}

// Block b of frame f: the quantised coefficients in zig-zag order (what the
// kernels compute with eight lanes and a transpose).
inline void block_coefficients(const uint8_t* f, const LjeGeom& g, const LjeTables& T, uint32_t b, int16_t out[64]) {
  const LjeBlock k = lje_block(g, b);
  int32_t ws[64];
  for (int r = 0; r < 8; ++r) {
    for (int c = 0; c < 8; ++c) ws[8 * r + c] = lje_sample(f, g, k.comp, 8 * k.br + r, 8 * k.bc + c);
    lje_fdct8<1>(ws + 8 * r);
  }
  for (int c = 0; c < 8; ++c) {
    int32_t col[8];
    for (int r = 0; r < 8; ++r) col[r] = ws[8 * r + c];
    lje_fdct8<2>(col);
    for (int r = 0; r < 8; ++r) {
      const int i = 8 * r + c;
      const int32_t q = lje_quant(col[r], T.div[k.comp ? 1 : 0][i]);
      out[T.pos[i]] = (int16_t)((k.dummy && i) ? 0 : q);
    }
  }
}

}  // namespace lje

#endif  // LM_JPEG_ENC_CORE_H
