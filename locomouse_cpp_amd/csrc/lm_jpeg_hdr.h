// lm_jpeg_hdr.h — JPEG header parsing shared by the host decoder
// (host/Jpeg.cpp) and the device decoder (lm_jpeg.hip); host code only.
//
// lmj::HeaderState holds what the segments in front of a scan define (DQT,
// DHT, SOF, DRI, JFIF / Adobe markers) and walks the stream exactly once:
// walk() calls `on_scan` at each SOS with the scan's components resolved, and
// the caller decodes (host/Jpeg.cpp) or records (lmj::parse below) the scan.
// Every rejection message is here, once.
//
// lmj::parse sorts a frame into one of three classes for the device decoder:
//   * rejected  — the host decoder refuses it, with the same message;
//   * in scope  — SOF0/SOF1, 8-bit samples and tables, grey or YCbCr at
//     4:4:4 / 4:2:2 / 4:2:0, one (interleaved) scan: lm_jpeg.hip decodes it;
//   * needs host — everything else the host decoder accepts.
// Failures before the first scan are rejections (the walk up to there is the
// host's own).  The device never decodes a scan to find where the next
// segment starts, so a failure behind the first scan — or a second scan —
// makes the frame "needs host": the host decoder has the last word on it.
#ifndef LM_JPEG_HDR_H
#define LM_JPEG_HDR_H

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "lm_jpeg_scan.h"

namespace lmj {

// Zig-zag scan position -> natural (row-major) coefficient index, padded so a
// corrupt run length past 63 lands on a harmless slot.
constexpr uint8_t kNatural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
    6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
    39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// ITU-T T.81 Annex K.3 tables (what MJPEG "AVI1" frames leave out).
constexpr uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Canonical Huffman table (T.81 C.2 / F.2.2.3) with a 9-bit lookahead: the
// device layout (LmjHuff) plus whether a DHT segment (or K.3) defined it.
struct HuffTable : LmjHuff {
  bool defined = false;
};

// False for an over-subscribed table (or one with an all-ones code).
inline bool build_huff(HuffTable& h, const uint8_t bits[16], const uint8_t* vals, int nvals) {
  int total = 0;
  for (int l = 0; l < 16; ++l) total += bits[l];
  if (total > 256 || total > nvals) return false;
  std::memset(h.look, 0, sizeof(h.look));
  std::memset(h.vals, 0, sizeof(h.vals));
  std::memset(h.maxcode, 0, sizeof(h.maxcode));
  std::memset(h.valoff, 0, sizeof(h.valoff));
  std::memcpy(h.vals, vals, (size_t)total);
  int code = 0, k = 0;
  h.maxcode[0] = -1;
  for (int l = 1; l <= 16; ++l) {
    h.valoff[l] = k - code;
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code)
      if (l <= LMJ_LOOK) {
        const int sh = LMJ_LOOK - l;
        for (int j = 0; j < (1 << sh); ++j)
          h.look[((code << sh) | j) & ((1 << LMJ_LOOK) - 1)] = (uint16_t)((l << 8) | vals[k]);
      }
    h.maxcode[l] = bits[l - 1] ? code - 1 : -1;
    if (bits[l - 1] && code >= (1 << l)) return false;  // over-subscribed (or an all-ones code)
    code <<= 1;
  }
  h.maxcode[17] = 0x7FFFFFFF;
  h.defined = true;
  return true;
}

// What SOF and SOS say about a component; a decoder derives from it.
struct CompBase {
  int id = 0, h = 1, v = 1, tq = 0;
  int td = 0, ta = 0;  // scan tables
  int dw = 0, dh = 0;  // downsampled size (jdinput.c: ceil(W * h / Hmax))
  int pitch = 0, prows = 0;
};

inline int u16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

template <class Comp>
struct HeaderState {
  uint16_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  bool q16[4] = {false, false, false, false};  // table given with 16-bit entries (Pq = 1)
  HuffTable dc[4], ac[4];
  int W = 0, H = 0, nc = 0, hmax = 1, vmax = 1, restart = 0;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  Comp comp[3];
  std::string why;

  bool fail(const char* m) {
    why = m;
    return false;
  }

  bool parse_dqt(const uint8_t* p, int n) {
    while (n > 0) {
      const int pq = p[0] >> 4, tq = p[0] & 15;
      const int sz = 1 + 64 * (pq ? 2 : 1);
      if (tq > 3 || pq > 1 || n < sz) return fail("bad DQT segment");
      for (int k = 0; k < 64; ++k) qt[tq][kNatural[k]] = (uint16_t)(pq ? u16(p + 1 + 2 * k) : p[1 + k]);
      qdef[tq] = true;
      q16[tq] = pq != 0;
      p += sz;
      n -= sz;
    }
    return true;
  }

  bool parse_dht(const uint8_t* p, int n) {
    while (n > 0) {
      if (n < 17) return fail("bad DHT segment");
      const int tc = p[0] >> 4, th = p[0] & 15;
      int total = 0;
      for (int l = 0; l < 16; ++l) total += p[1 + l];
      if (tc > 1 || th > 3 || total > 256 || n < 17 + total) return fail("bad DHT segment");
      if (!build_huff(tc ? ac[th] : dc[th], p + 1, p + 17, total)) return fail("bad Huffman table");
      p += 17 + total;
      n -= 17 + total;
    }
    return true;
  }

  bool parse_sof(const uint8_t* p, int n) {
    if (sof) return fail("more than one frame header");
    if (n < 6) return fail("bad SOF segment");
    if (p[0] != 8) return fail("only 8-bit JPEG samples are supported");
    H = u16(p + 1);
    W = u16(p + 3);
    nc = p[5];
    if (W <= 0 || H <= 0) return fail("JPEG image of zero size (DNL not supported)");
    if (nc != 1 && nc != 3) return fail("only 1- or 3-component JPEG images are supported");
    if (n < 6 + 3 * nc) return fail("bad SOF segment");
    hmax = vmax = 1;
    for (int c = 0; c < nc; ++c) {
      Comp& C = comp[c];
      C.id = p[6 + 3 * c];
      C.h = p[7 + 3 * c] >> 4;
      C.v = p[7 + 3 * c] & 15;
      C.tq = p[8 + 3 * c];
      if (C.h < 1 || C.h > 4 || C.v < 1 || C.v > 4 || C.tq > 3) return fail("bad JPEG component parameters");
      hmax = std::max(hmax, C.h);
      vmax = std::max(vmax, C.v);
    }
    const int mcux = (W + 8 * hmax - 1) / (8 * hmax), mcuy = (H + 8 * vmax - 1) / (8 * vmax);
    for (int c = 0; c < nc; ++c) {
      Comp& C = comp[c];
      C.dw = (W * C.h + hmax - 1) / hmax;
      C.dh = (H * C.v + vmax - 1) / vmax;
      C.pitch = mcux * C.h * 8;
      C.prows = mcuy * C.v * 8;
    }
    sof = true;
    return true;
  }

  // Colour space as libjpeg's default_decompress_parms picks it.
  bool is_rgb() const {
    if (nc != 3) return false;
    if (jfif) return false;
    if (adobe) return adobe_transform == 0;
    return comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B';
  }

  // Component c's plane feeds channel 0 of the BGR rendering?
  bool needed(int c) const { return nc == 1 || (is_rgb() ? c == 2 : c <= 1); }

  void fill_default_tables() {
    if (!dc[0].defined) build_huff(dc[0], kDcLumBits, kDcVals, 12);
    if (!dc[1].defined) build_huff(dc[1], kDcChromBits, kDcVals, 12);
    if (!ac[0].defined) build_huff(ac[0], kAcLumBits, kAcLumVals, 162);
    if (!ac[1].defined) build_huff(ac[1], kAcChromBits, kAcChromVals, 162);
  }

  // The standard tables for what DHT left out, then what every scan needs defined.
  bool check_scan_tables(int ns, const int* idx) {
    fill_default_tables();
    for (int i = 0; i < ns; ++i) {
      const Comp& C = comp[idx[i]];
      if (!dc[C.td].defined || !ac[C.ta].defined) return fail("scan uses an undefined Huffman table");
      if (needed(idx[i]) && !qdef[C.tq]) return fail("component uses an undefined quantisation table");
    }
    return true;
  }

  // Walks the segments.  At each SOS, with the scan's components in idx[0..ns)
  // and their td / ta set: on_scan(data, end, ns, idx, first) returns where the
  // walk goes on (the marker behind the entropy-coded segment), or nullptr
  // after fail().
  template <class OnScan>
  bool walk(const uint8_t* d, size_t n, OnScan&& on_scan) {
    const uint8_t* end = d + n;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("not a JPEG image (no SOI)");
    const uint8_t* p = d + 2;
    bool scanned = false;
    for (;;) {
      while (p < end && *p != 0xFF) ++p;  // garbage between segments
      while (p < end && *p == 0xFF) ++p;
      if (p >= end) break;
      const int m = *p++;
      if (m == 0xD9) break;                                 // EOI
      if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // TEM / stray RSTn
      if (m == 0xD8) return fail("nested SOI");
      if (end - p < 2) return fail("truncated JPEG segment");
      const int len = u16(p);
      if (len < 2 || end - p < len) return fail("truncated JPEG segment");
      const uint8_t* s = p + 2;
      const int sn = len - 2;
      p += len;
      switch (m) {
        case 0xC0:
        case 0xC1:
          if (!parse_sof(s, sn)) return false;
          break;
        case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7:
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
          return fail("only sequential Huffman JPEG is supported (progressive/lossless/arithmetic found)");
        case 0xC4:
          if (!parse_dht(s, sn)) return false;
          break;
        case 0xDB:
          if (!parse_dqt(s, sn)) return false;
          break;
        case 0xDD:
          if (sn < 2) return fail("bad DRI segment");
          restart = u16(s);
          break;
        case 0xE0:
          if (sn >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
          break;
        case 0xEE:
          if (sn >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
            adobe = true;
            adobe_transform = s[11];
          }
          break;
        case 0xDA: {
          if (!sof) return fail("scan before frame header");
          if (sn < 1) return fail("bad SOS segment");
          const int ns = s[0];
          if (ns < 1 || ns > nc || sn < 1 + 2 * ns + 3) return fail("bad SOS segment");
          int idx[3] = {0, 0, 0};
          for (int i = 0; i < ns; ++i) {
            const int cid = s[1 + 2 * i];
            int c = 0;
            while (c < nc && comp[c].id != cid) ++c;
            if (c == nc) return fail("scan names an unknown component");
            idx[i] = c;
            comp[c].td = s[2 + 2 * i] >> 4;
            comp[c].ta = s[2 + 2 * i] & 15;
            if (comp[c].td > 3 || comp[c].ta > 3) return fail("bad SOS table selector");
          }
          p = on_scan(p, end, ns, idx, !scanned);
          if (!p) return false;
          scanned = true;
          break;
        }
        default:
          break;  // APPn, COM, DNL, ...
      }
    }
    if (!scanned) return fail("JPEG image has no scan");
    return true;
  }
};

// ------------------------------------------------- the device decoder's view
enum Class { kInScope = 0, kNeedsHost = 1, kRejected = 2 };

struct Header {
  Class cls = kRejected;
  std::string why;       // rejection message (the host decoder's), or why the host is needed
  int W = 0, H = 0, nc = 0;
  int h[3] = {1, 1, 1}, v[3] = {1, 1, 1};
  int restart = 0;
  size_t scan_off = 0, scan_len = 0;  // the first scan's entropy-coded bytes
  uint16_t qt[2][64];                 // Y and Cb tables, natural order (in scope only)
  LmjHuff huff[6];                    // DC, AC of each scan component (in scope only)
};

// End of the entropy-coded segment that starts at p: the first FF followed by
// anything but 00 or D0..D7, or the end of the data.  (FF FF — a fill byte —
// ends it too: the lanes then find too few blocks and the host decodes the
// frame, whose reader skips fill bytes.)
// rst (may be null): the marker index of the segment, the offset from its
// start of the byte behind each FF D0..D7, in order (the interval path of the
// device decoder starts a lane at each).
inline const uint8_t* scan_end(const uint8_t* p, const uint8_t* end, std::vector<uint32_t>* rst = nullptr) {
  const uint8_t* const start = p;
  while (p < end) {
    if (p[0] == 0xFF && p + 1 < end && p[1] != 0) {
      if (!(p[1] >= 0xD0 && p[1] <= 0xD7)) return p;
      if (rst) rst->push_back((uint32_t)(p + 2 - start));
    }
    ++p;
  }
  return end;
}

inline void parse(const uint8_t* d, size_t n, Header& out, std::vector<uint32_t>* rst = nullptr) {
  out = Header();
  if (rst) rst->clear();
  HeaderState<CompBase> S;
  bool seen = false;
  const char* host_why = nullptr;
  const bool ok = S.walk(d, n, [&](const uint8_t* p, const uint8_t* end, int ns, const int* idx, bool first) {
    if (!first) {
      host_why = "more than one scan";
      return scan_end(p, end);
    }
    if (!S.check_scan_tables(ns, idx)) return (const uint8_t*)nullptr;
    seen = true;
    const int nc = S.nc;
    out.W = S.W;
    out.H = S.H;
    out.nc = nc;
    out.restart = S.restart;
    for (int c = 0; c < nc; ++c) {
      out.h[c] = S.comp[c].h;
      out.v[c] = S.comp[c].v;
    }
    out.scan_off = (size_t)(p - d);
    const uint8_t* e = scan_end(p, end, rst);
    out.scan_len = (size_t)(e - p);
    const CompBase* C = S.comp;
    if (S.is_rgb()) host_why = "RGB (Adobe) colour space";
    else if (ns != nc) host_why = "more than one scan";
    else if (nc == 3 && !(idx[0] == 0 && idx[1] == 1 && idx[2] == 2)) host_why = "scan components out of order";
    // (a single component's scan is one block per MCU whatever its sampling factors say)
    else if (nc == 3 && !(C[1].h == 1 && C[1].v == 1 && C[2].h == 1 && C[2].v == 1 &&
                          ((C[0].h == 1 && C[0].v == 1) || (C[0].h == 2 && C[0].v <= 2))))
      host_why = "sampling factors out of scope";
    else if (S.q16[C[0].tq] || (nc == 3 && S.q16[C[1].tq])) host_why = "16-bit quantisation tables";
    if (!host_why) {
      std::memcpy(out.qt[0], S.qt[C[0].tq], sizeof(out.qt[0]));
      std::memcpy(out.qt[1], S.qt[C[nc == 3 ? 1 : 0].tq], sizeof(out.qt[1]));
      for (int c = 0; c < 3; ++c) {
        const CompBase& K = C[c < nc ? c : 0];
        out.huff[2 * c] = S.dc[K.td];
        out.huff[2 * c + 1] = S.ac[K.ta];
      }
    }
    return e;
  });
  if (!ok) {
    out.cls = seen ? kNeedsHost : kRejected;
    out.why = seen ? "data after the first scan" : S.why;
    return;
  }
  out.cls = host_why ? kNeedsHost : kInScope;
  out.why = host_why ? host_why : "";
}

// The scan description the lanes work from (d is set by the caller).
inline LmjScan make_scan(const Header& h, uint32_t subseq) {
  LmjScan sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.len = (uint32_t)h.scan_len;
  sc.subseq = subseq;
  sc.nsub = (uint32_t)((h.scan_len + subseq - 1) / subseq);
  sc.restart = (uint32_t)h.restart;
  sc.nc = (uint8_t)h.nc;
  sc.hx = (uint8_t)(h.nc == 3 ? h.h[0] : 1);
  sc.vx = (uint8_t)(h.nc == 3 ? h.v[0] : 1);
  sc.bpm = (uint8_t)(h.nc == 3 ? sc.hx * sc.vx + 2 : 1);
  const LmjPlanes P = lmj_planes(h.W, h.H, h.nc, sc.hx, sc.vx);
  sc.nblk = (uint32_t)P.mcux * (uint32_t)P.mcuy * sc.bpm;
  return sc;
}

inline void make_tables(const Header& h, LmjTableSet& T) {
  std::memset(&T, 0, sizeof(T));
  for (int i = 0; i < 6; ++i) T.t[i] = h.huff[i];
  std::memcpy(T.nat, kNatural, 64);
}

}  // namespace lmj

#endif  // LM_JPEG_HDR_H
