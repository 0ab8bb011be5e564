// lm_jpeg_scan.h — baseline JPEG decoding split so that one frame's entropy
// scan can be decoded by many lanes at once ("Device JPEG decode").
// Host and device compile the same code: lm_jpeg.hip runs it one subsequence
// per GPU lane, lmj_scan_frame_host() runs the same lanes one after another on
// the CPU (tests/cpp/jpeg_harness.cpp, tests/cpp/jpeg_scan_fuzz.cpp).
//
// The arithmetic restates host/Jpeg.cpp (T.81 F.2.2 Huffman decoding, libjpeg's
// ISLOW IDCT, fancy h2v1 / h2v2 upsampling, jdcolor.c's Cb -> B term); header
// parsing is shared with it (lm_jpeg_hdr.h) and decides which frames this
// path may take.
//
// The scan scheme (self-synchronising subsequences):
//   * the entropy-coded segment is cut into subsequences of S bytes; a lane
//     owns the symbols that START inside its subsequence;
//   * a decoder's state is (bit position p, zig-zag index k, block-in-MCU b);
//     DC prediction is not part of it (DC differences are summed afterwards);
//   * lanes first decode from a guessed state (start of a block at their first
//     byte), then re-decode from their left neighbour's exit state until no
//     exit state changes.  Lane 0 of a chunk starts from the true state, so
//     round r settles lane r at the latest: rounds <= lanes - 1;
//   * a final pass with the settled states writes the coefficients.
//
// Bounds, for any input bytes: every loop of lmj_decode_subseq advances p by
// at least one bit (or jumps forward past a marker) and is capped by the bits
// of the subsequence; every table index is masked or range-checked; every
// coefficient write is guarded by the frame's block count; every byte read is
// guarded by the scan's length.
#ifndef LM_JPEG_SCAN_H
#define LM_JPEG_SCAN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LMJ_HD __host__ __device__ inline
#else
#define LMJ_HD inline
#endif

#if defined(__clang__)
#define LMJ_UNROLL _Pragma("unroll")
#else
#define LMJ_UNROLL
#endif

#define LMJ_LOOK 9            // Huffman lookahead bits (as host/Jpeg.cpp)
#define LMJ_MAX_BPM 6         // blocks per MCU in scope: 4 Y + Cb + Cr
#define LMJ_LANES 128         // subsequences one workgroup decodes at once (a chunk)
#define LMJ_SUBSEQ_MIN 4      // smallest subsequence, bytes
#define LMJ_SUBSEQ_DEFAULT 64

// Error bits a lane can raise in the final pass; any of them sends the frame
// back to the host decoder.
#define LMJ_E_CODE 1u      // not a Huffman code
#define LMJ_E_RUN 2u       // run length past coefficient 63
#define LMJ_E_DCSIZE 4u    // DC size category above 16
#define LMJ_E_RST 8u       // restart marker off an interval boundary (or without DRI)
#define LMJ_E_TRUNC 16u    // data ended inside a block or MCU
#define LMJ_E_BLOCKS 32u   // block count differs from the frame's

// Canonical Huffman table with a 9-bit lookahead, device layout.
struct LmjHuff {
  uint16_t look[1 << LMJ_LOOK];  // (length << 8) | symbol; 0 = longer code
  int32_t maxcode[18];           // largest code of each length, -1 if none
  int32_t valoff[18];            // symbol index = code + valoff[length]
  uint8_t vals[256];
};

// The tables of one scan: DC then AC table of each component, and the zig-zag
// order (kept with them so that device code reads it from LDS).
struct LmjTableSet {
  LmjHuff t[6];
  uint8_t nat[64];
};

struct LmjState {
  uint32_t p;  // bit position in the scan (byte * 8 + bit), stuffed bytes counted
  uint16_t k;  // next zig-zag index (0: the DC symbol comes next)
  uint16_t b;  // block within the MCU
};
LMJ_HD bool lmj_same(const LmjState& a, const LmjState& b) { return a.p == b.p && a.k == b.k && a.b == b.b; }

struct LmjLane {  // what a lane's decode produced from its entry state
  uint32_t nblk;  // blocks completed
  uint32_t nrst;  // restart markers passed
  uint32_t err;   // LMJ_E_* (final pass)
};

// One frame's scan as the lanes see it.
struct LmjScan {
  const uint8_t* d;   // entropy-coded bytes
  uint32_t len;
  uint32_t subseq;    // S
  uint32_t nsub;      // ceil(len / S)
  uint32_t nblk;      // blocks the frame has, in scan order
  uint32_t restart;   // MCUs per restart interval, 0 = none
  uint8_t bpm;        // blocks per MCU
  uint8_t nc;         // 1 or 3
  uint8_t hx, vx;     // luma blocks per MCU across / down (1 for grey)
  uint8_t pad[4];
};

// Component of block r of the MCU: hx * vx luma blocks, then Cb, then Cr.
LMJ_HD uint32_t lmj_comp_of(const LmjScan& sc, uint32_t r) {
  if (sc.nc != 3) return 0;
  const uint32_t ny = (uint32_t)sc.hx * sc.vx;
  return r < ny ? 0u : r == ny ? 1u : 2u;
}

// ---------------------------------------------------------------- bit reader
// Byte stuffing (FF 00) is removed here; FF followed by anything else is a
// marker, which ends the bits.  All reads are below len.
LMJ_HD bool lmj_marker_at(const uint8_t* d, uint32_t len, uint32_t q) {
  return q < len && d[q] == 0xFF && !(q + 1 < len && d[q + 1] == 0);
}

// 32 bits from (pos, bit), zero filled; avail = how many of them are data,
// stop = where the data ends (a marker's FF, or len) when avail < 32.
LMJ_HD uint32_t lmj_peek(const uint8_t* d, uint32_t len, uint32_t pos, uint32_t bit, int& avail, uint32_t& stop) {
  uint64_t acc = 0;
  int n = 0;
  uint32_t q = pos;
  for (int i = 0; i < 5; ++i) {
    if (q >= len) break;
    const uint32_t v = d[q];
    if (v == 0xFF) {
      if (q + 1 < len && d[q + 1] == 0) q += 2;
      else break;
    } else {
      q += 1;
    }
    acc = (acc << 8) | v;
    n += 8;
  }
  stop = q;
  acc <<= (40 - n);
  avail = n - (int)bit;
  if (avail < 0) avail = 0;
  if (avail > 32) avail = 32;
  return (uint32_t)((acc >> (8 - bit)) & 0xFFFFFFFFu);
}

// Steps (pos, bit) forward by n <= 32 bits that lmj_peek reported as data.
LMJ_HD void lmj_advance(const uint8_t* d, uint32_t len, uint32_t& pos, uint32_t& bit, uint32_t n) {
  bit += n;
  for (int i = 0; i < 5 && bit >= 8; ++i) {
    if (pos >= len || lmj_marker_at(d, len, pos)) break;
    pos += (d[pos] == 0xFF) ? 2u : 1u;  // (a data FF is followed by its stuffed 00)
    bit -= 8;
  }
  if (bit >= 8) bit = 0;  // unreachable for n <= avail
}

// A lane's guess: the start of a block at the first byte of subsequence i
// (stepping off a stuffed 00 or the second byte of a restart marker when the
// boundary falls between the two).
LMJ_HD LmjState lmj_guess(const LmjScan& sc, uint32_t i) {
  uint32_t pos = i * sc.subseq;
  if (pos > 0 && pos < sc.len && sc.d[pos - 1] == 0xFF && (sc.d[pos] == 0 || (sc.d[pos] >= 0xD0 && sc.d[pos] <= 0xD7)))
    pos += 1;
  LmjState s;
  s.p = pos * 8;
  s.k = 0;
  s.b = 0;
  return s;
}

LMJ_HD uint32_t lmj_end_bit(const LmjScan& sc, uint32_t i) {
  const uint64_t e = (uint64_t)(i + 1) * sc.subseq;
  return (uint32_t)(e < sc.len ? e : sc.len) * 8u;
}

LMJ_HD int lmj_extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// Decodes the symbols that start in [s.p, end_bit) from state s; returns the
// exit state.  WRITE: also stores AC coefficients (int16, natural order) and
// DC differences (int32) of the blocks from first_blk on, and checks restart
// markers against the interval (first_rst = markers passed before this lane).
template <bool WRITE>
LMJ_HD LmjState lmj_decode_subseq(const LmjScan& sc, const LmjTableSet& T, LmjState s, uint32_t end_bit,
                                  uint32_t first_blk, uint32_t first_rst, int16_t* coef, int32_t* dcdiff,
                                  LmjLane& o) {
  o.nblk = 0;
  o.nrst = 0;
  o.err = 0;
  if (s.p >= end_bit) return s;
  if (s.b >= sc.bpm) s.b = 0;
  if (s.k > 63) s.k = 0;
  const uint32_t cap = end_bit - s.p + 1;  // every turn moves p forward by a bit or more
  for (uint32_t turn = 0; turn < cap && s.p < end_bit; ++turn) {
    uint32_t pos = s.p >> 3, bit = s.p & 7;
    int avail;
    uint32_t stop;
    const uint32_t w = lmj_peek(sc.d, sc.len, pos, bit, avail, stop);
    const uint32_t c = lmj_comp_of(sc, s.b);
    const LmjHuff& H = T.t[c * 2 + (s.k ? 1 : 0)];
    int l, sym;
    bool bad = false;
    const uint32_t e = H.look[w >> (32 - LMJ_LOOK)];
    if (e >> 8) {
      l = (int)(e >> 8);
      sym = (int)(e & 255);
    } else {
      l = LMJ_LOOK + 1;
      int32_t code = (int32_t)(w >> (32 - l));
      while (l <= 16 && code > H.maxcode[l]) {
        ++l;
        code = (int32_t)(w >> (32 - (l <= 16 ? l : 16)));
      }
      if (l > 16) {  // not a code: the host takes 16 bits and symbol 0
        bad = true;
        l = 16;
        sym = 0;
      } else {
        sym = H.vals[(code + H.valoff[l]) & 255];
      }
    }
    const int sz = s.k ? (sym & 15) : (sym > 16 ? 16 : sym);
    if (l + sz > avail) {  // the symbol runs into a marker or the end of the data
      const bool clean = s.k == 0 && s.b == 0;
      if (stop + 1 < sc.len && sc.d[stop] == 0xFF && sc.d[stop + 1] >= 0xD0 && sc.d[stop + 1] <= 0xD7) {
        if (WRITE) {
          const uint64_t want = (uint64_t)(first_rst + o.nrst + 1) * sc.restart * sc.bpm;
          if (!clean || sc.restart == 0 || (uint64_t)(first_blk + o.nblk) != want) o.err |= LMJ_E_RST;
        }
        ++o.nrst;
        s.p = (stop + 2) * 8;  // a true synchronisation point
        s.k = 0;
        s.b = 0;
      } else {
        if (WRITE && !clean) o.err |= LMJ_E_TRUNC;
        s.p = sc.len * 8;  // nothing more to decode, for this lane and all after it
      }
      continue;
    }
    if (WRITE && bad) o.err |= LMJ_E_CODE;
    const uint32_t extra = sz ? ((w << l) >> (32 - sz)) : 0;
    lmj_advance(sc.d, sc.len, pos, bit, (uint32_t)(l + sz));
    s.p = pos * 8 + bit;
    const uint32_t blk = first_blk + o.nblk;
    const bool store = WRITE && blk < sc.nblk && c < 2;  // Cr is decoded for its state only
    if (s.k == 0) {
      if (WRITE && sym > 16) o.err |= LMJ_E_DCSIZE;
      if (store) dcdiff[blk] = sz ? lmj_extend(extra, sz) : 0;
      s.k = 1;
    } else {
      const int r = sym >> 4;
      if (sz) {
        int k = s.k + r;
        if (k > 63) {
          if (WRITE) o.err |= LMJ_E_RUN;
          k = 63;
        }
        if (store) coef[(uint64_t)blk * 64 + T.nat[k & 63]] = (int16_t)lmj_extend(extra, sz);
        s.k = (uint16_t)(k + 1);
      } else if (r == 15) {
        s.k = (uint16_t)(s.k + 16);
      } else {
        s.k = 64;  // end of block
      }
    }
    if (s.k >= 64) {
      s.k = 0;
      s.b = (uint16_t)(s.b + 1 == sc.bpm ? 0 : s.b + 1);
      ++o.nblk;
    }
  }
  return s;
}

// Restart markers a clean scan holds: one between consecutive intervals.
LMJ_HD uint32_t lmj_expected_rst(const LmjScan& sc) {
  const uint32_t mcus = sc.bpm ? sc.nblk / sc.bpm : 0;
  return sc.restart && mcus ? (mcus - 1) / sc.restart : 0;
}

// ------------------------------------------------------------ interval path
// A scan with restart markers needs no guess: behind RSTn the state is known
// (a byte boundary, k = 0, b = 0) and DC prediction starts again, so every
// restart interval decodes on its own.  Lane j of a frame with `nint`
// intervals (lmj_expected_rst + 1) decodes the bytes [start, end): start is the
// byte behind marker j - 1 (0 for lane 0), end the byte behind marker j (the
// scan's length for the last lane), both from the marker index, which must
// hold exactly lmj_expected_rst entries.  Its first block is j * restart * bpm.
// It returns true when the lane completed exactly its blocks, cleanly: no error
// bit, the block count of its interval, its one marker passed (none for the
// last lane) at a block boundary.  Anything else hands the frame to the
// subsequence path, which then decodes it as if this path had not run.
// The loop is lmj_decode_subseq's, with its bit cap and bounds checks.
LMJ_HD bool lmj_decode_interval(const LmjScan& sc, const LmjTableSet& T, uint32_t j, uint32_t nint, uint32_t start,
                                uint32_t end, int16_t* coef, int32_t* dcdiff) {
  if (sc.restart == 0 || j >= nint || start > end || end > sc.len) return false;
  const uint64_t per = (uint64_t)sc.restart * sc.bpm, first = (uint64_t)j * per;
  if (first >= sc.nblk) return false;
  const uint32_t want = (uint32_t)(sc.nblk - first < per ? sc.nblk - first : per);
  const bool last = j + 1 == nint;
  LmjState s;
  s.p = start * 8u;
  s.k = 0;
  s.b = 0;
  LmjLane o;
  s = lmj_decode_subseq<true>(sc, T, s, end * 8u, (uint32_t)first, j, coef, dcdiff, o);
  return o.err == 0 && o.nblk == want && o.nrst == (last ? 0u : 1u) && s.k == 0 && s.b == 0;
}

// DC prediction restarts at block `blk` of the scan?
LMJ_HD bool lmj_dc_reset(const LmjScan& sc, uint32_t blk) {
  return sc.restart && blk % (sc.restart * sc.bpm) == 0;
}

// ------------------------------------------------------------------- planes
struct LmjPlanes {  // component planes padded to whole MCUs, as the host's
  int mcux, mcuy;
  int pitch_y, rows_y, pitch_c, rows_c;
  int dw_c, dh_c;  // chroma plane's real size
};

LMJ_HD LmjPlanes lmj_planes(int W, int H, int nc, int hx, int vx) {
  LmjPlanes P;
  if (nc == 1) hx = vx = 1;
  P.mcux = (W + 8 * hx - 1) / (8 * hx);
  P.mcuy = (H + 8 * vx - 1) / (8 * vx);
  P.pitch_y = P.mcux * hx * 8;
  P.rows_y = P.mcuy * vx * 8;
  P.pitch_c = P.mcux * 8;
  P.rows_c = P.mcuy * 8;
  P.dw_c = (W + hx - 1) / hx;
  P.dh_c = (H + vx - 1) / vx;
  return P;
}

// Where block `blk` of the scan goes: component and its 8x8 position.
LMJ_HD void lmj_block_pos(const LmjScan& sc, const LmjPlanes& P, uint32_t blk, int& comp, int& bx, int& by) {
  const uint32_t mcu = blk / sc.bpm, r = blk % sc.bpm;
  const int mx = (int)(mcu % (uint32_t)P.mcux), my = (int)(mcu / (uint32_t)P.mcux);
  comp = (int)lmj_comp_of(sc, r);
  if (comp == 0 && sc.nc == 3) {
    bx = mx * sc.hx + (int)(r % sc.hx);
    by = my * sc.vx + (int)(r / sc.hx);
  } else {
    bx = mx;
    by = my;
  }
}

// ---------------------------------------------------------------- ISLOW IDCT
// host/Jpeg.cpp's idct_islow (jidctint.c): 64-bit products throughout — a
// decodable coefficient reaches 2^15 and an 8-bit table 255, so the even part
// alone ((z2 + z3) * F0541 on 2^24 operands, shifted sums of 2^23 << 13) passes
// 2^31.  The range limit table is restated as arithmetic.
LMJ_HD uint8_t lmj_range(int64_t x) {
  const int i = (int)x & 1023;
  return (uint8_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}
LMJ_HD int64_t lmj_descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }
LMJ_HD int64_t lmj_shl(int64_t a, int b) { return (int64_t)((uint64_t)a << b); }

LMJ_HD void lmj_idct_islow(const int16_t* coef, const uint16_t* q, uint8_t* out, int pitch) {
  const int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  const int kConstBits = 13, kPass1 = 2;
  int32_t ws[64];  // (both loops unrolled on the device: the workspace stays in registers)
  LMJ_UNROLL
  for (int c = 0; c < 8; ++c) {
    const int16_t* in = coef + c;
    const uint16_t* qq = q + c;
    int32_t* w = ws + c;
    if (!(in[8] | in[16] | in[24] | in[32] | in[40] | in[48] | in[56])) {
      const int32_t dc = (int32_t)lmj_shl((int32_t)in[0] * (int32_t)qq[0], kPass1);
      LMJ_UNROLL
      for (int r = 0; r < 8; ++r) w[8 * r] = dc;
      continue;
    }
    int64_t z2 = (int32_t)in[16] * (int32_t)qq[16], z3 = (int32_t)in[48] * (int32_t)qq[48];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
    z2 = (int32_t)in[0] * (int32_t)qq[0];
    z3 = (int32_t)in[32] * (int32_t)qq[32];
    int64_t tmp0 = lmj_shl(z2 + z3, kConstBits), tmp1 = lmj_shl(z2 - z3, kConstBits);
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
    const int s = kConstBits - kPass1;
    w[0] = (int32_t)lmj_descale(t10 + tmp3, s);
    w[56] = (int32_t)lmj_descale(t10 - tmp3, s);
    w[8] = (int32_t)lmj_descale(t11 + tmp2, s);
    w[48] = (int32_t)lmj_descale(t11 - tmp2, s);
    w[16] = (int32_t)lmj_descale(t12 + tmp1, s);
    w[40] = (int32_t)lmj_descale(t12 - tmp1, s);
    w[24] = (int32_t)lmj_descale(t13 + tmp0, s);
    w[32] = (int32_t)lmj_descale(t13 - tmp0, s);
  }
  const int s2 = kConstBits + kPass1 + 3;
  LMJ_UNROLL
  for (int r = 0; r < 8; ++r) {
    const int32_t* w = ws + 8 * r;
    uint8_t* o = out + (int64_t)r * pitch;
    if (!(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7])) {
      const uint8_t v = lmj_range(lmj_descale(w[0], kPass1 + 3));
      for (int x = 0; x < 8; ++x) o[x] = v;
      continue;
    }
    int64_t z2 = w[2], z3 = w[6];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
    int64_t tmp0 = lmj_shl((int64_t)w[0] + w[4], kConstBits), tmp1 = lmj_shl((int64_t)w[0] - w[4], kConstBits);
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
    o[0] = lmj_range(lmj_descale(t10 + tmp3, s2));
    o[7] = lmj_range(lmj_descale(t10 - tmp3, s2));
    o[1] = lmj_range(lmj_descale(t11 + tmp2, s2));
    o[6] = lmj_range(lmj_descale(t11 - tmp2, s2));
    o[2] = lmj_range(lmj_descale(t12 + tmp1, s2));
    o[5] = lmj_range(lmj_descale(t12 - tmp1, s2));
    o[3] = lmj_range(lmj_descale(t13 + tmp0, s2));
    o[4] = lmj_range(lmj_descale(t13 - tmp0, s2));
  }
}

// ------------------------------------------------- upsampling and channel 0
// Chroma sample at full-resolution (x, y): libjpeg's fancy h2v1 / h2v2
// triangle filters with the host's edge rules (Decoder::upsample_row).
LMJ_HD int lmj_chroma_at(const uint8_t* P, const LmjPlanes& L, int hx, int vx, int x, int y) {
  if (hx == 1) return P[(int64_t)y * L.pitch_c + x];  // 4:4:4 (vx is 1 in scope)
  const int dw = L.dw_c, cx = x >> 1;
  if (vx == 2) {
    const int r = y >> 1;
    const int r2 = (y & 1) ? (r + 1 < L.dh_c - 1 ? r + 1 : L.dh_c - 1) : (r - 1 > 0 ? r - 1 : 0);
    const uint8_t* a = P + (int64_t)r * L.pitch_c;
    const uint8_t* b = P + (int64_t)r2 * L.pitch_c;
    const int t = 3 * a[cx] + b[cx];
    if (x & 1) {
      if (cx == dw - 1) return (t * 4 + 7) >> 4;
      return (t * 3 + 3 * a[cx + 1] + b[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (t * 4 + 8) >> 4;
    return (t * 3 + 3 * a[cx - 1] + b[cx - 1] + 8) >> 4;
  }
  const uint8_t* a = P + (int64_t)y * L.pitch_c;
  if (x & 1) {
    if (cx == dw - 1) return a[cx];
    return (a[cx] * 3 + a[cx + 1] + 2) >> 2;
  }
  if (cx == 0) return a[0];
  return (a[cx] * 3 + a[cx - 1] + 1) >> 2;
}

// Channel 0 of the BGR rendering: Y for a grey frame, else
// clamp(Y + ((1.772 * 2^16 * (Cb - 128) + 2^15) >> 16)) (jdcolor.c).
LMJ_HD uint8_t lmj_channel0(const uint8_t* Y, const uint8_t* Cb, const LmjPlanes& L, int nc, int hx, int vx, int x,
                            int y) {
  const int yy = Y[(int64_t)y * L.pitch_y + x];
  if (nc == 1) return (uint8_t)yy;
  const int cb = lmj_chroma_at(Cb, L, hx, vx, x, y);
  const int32_t fix = 116130;  // (int32_t)(1.772 * 65536.0 + 0.5)
  const int b = yy + (int)((int16_t)((fix * (cb - 128) + (1 << 15)) >> 16));
  return (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
}

// ------------------------------------------------------ host run of the lanes
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

struct LmjScanStats {
  uint32_t subsequences = 0, rounds = 0, max_rounds = 0, err = 0;
};

// The kernel's schedule on the CPU: chunks of `lanes` subsequences, lane by
// lane, round by round.  coef: nblk * 64 int16, zeroed here; dcdiff: nblk.
// Returns the error bits (0: the scan decoded cleanly into exactly nblk blocks).
inline uint32_t lmj_scan_frame_host(const LmjScan& sc, const LmjTableSet& T, int lanes, int16_t* coef, int32_t* dcdiff,
                                    LmjScanStats* st) {
  for (uint64_t i = 0; i < (uint64_t)sc.nblk * 64; ++i) coef[i] = 0;
  for (uint32_t i = 0; i < sc.nblk; ++i) dcdiff[i] = 0;
  std::vector<LmjState> in((size_t)lanes), ex((size_t)lanes), nx((size_t)lanes);
  std::vector<LmjLane> ln((size_t)lanes);
  LmjState carry{0, 0, 0};
  uint32_t blk0 = 0, rst0 = 0, err = 0, rounds = 0, max_rounds = 0;
  for (uint32_t base = 0; base < sc.nsub; base += (uint32_t)lanes) {
    const int m = (int)(sc.nsub - base < (uint32_t)lanes ? sc.nsub - base : (uint32_t)lanes);
    for (int t = 0; t < m; ++t) {
      in[t] = t == 0 ? carry : lmj_guess(sc, base + t);
      ex[t] = lmj_decode_subseq<false>(sc, T, in[t], lmj_end_bit(sc, base + t), 0, 0, nullptr, nullptr, ln[t]);
    }
    uint32_t r = 0;
    bool settled = false;
    // Lane 0 is right from the start and round r settles lane r at the latest,
    // so m - 1 rounds always suffice, whether or not the last one saw a change.
    while (r + 1 < (uint32_t)m && !settled) {
      ++r;
      bool changed = false;
      for (int t = 0; t < m; ++t) nx[t] = ex[t];
      for (int t = 1; t < m; ++t) {
        if (lmj_same(ex[t - 1], in[t])) continue;
        in[t] = ex[t - 1];
        nx[t] = lmj_decode_subseq<false>(sc, T, in[t], lmj_end_bit(sc, base + t), 0, 0, nullptr, nullptr, ln[t]);
        if (!lmj_same(nx[t], ex[t])) changed = true;
      }
      for (int t = 0; t < m; ++t) ex[t] = nx[t];
      settled = !changed;
    }
    rounds += r;
    if (r > max_rounds) max_rounds = r;
    for (int t = 0; t < m; ++t) {
      LmjLane o;
      const uint32_t nb = ln[t].nblk, nr = ln[t].nrst;
      lmj_decode_subseq<true>(sc, T, in[t], lmj_end_bit(sc, base + t), blk0, rst0, coef, dcdiff, o);
      err |= o.err;
      blk0 += nb;
      rst0 += nr;
    }
    carry = ex[m - 1];
  }
  if (blk0 != sc.nblk || carry.k != 0 || carry.b != 0) err |= LMJ_E_BLOCKS;
  if (rst0 != lmj_expected_rst(sc)) err |= LMJ_E_RST;  // a marker the interval asks for is missing
  if (st) {
    st->subsequences = sc.nsub;
    st->rounds = rounds;
    st->max_rounds = max_rounds;
    st->err = err;
  }
  return err;
}

// The interval path's schedule on the CPU, lane by lane (k_jpeg_scan_rst).
// rst: the scan's marker index (lmj::scan_end), nrst entries.  coef and dcdiff
// as above, zeroed here.  Returns true when the path finished the frame; false
// hands it to lmj_scan_frame_host: the index count differs from the expected
// count, the frame has a single interval, or some lane did not complete exactly
// its blocks.  (coef and dcdiff then hold what the lanes left: zero them again,
// as lmj_scan_frame_host does.)
inline bool lmj_scan_intervals_host(const LmjScan& sc, const LmjTableSet& T, const uint32_t* rst, uint32_t nrst,
                                    int16_t* coef, int32_t* dcdiff) {
  for (uint64_t i = 0; i < (uint64_t)sc.nblk * 64; ++i) coef[i] = 0;
  for (uint32_t i = 0; i < sc.nblk; ++i) dcdiff[i] = 0;
  const uint32_t expected = lmj_expected_rst(sc);
  if (expected == 0 || nrst != expected) return false;
  const uint32_t nint = expected + 1;
  bool ok = true;
  for (uint32_t j = 0; j < nint; ++j)  // every lane runs, as on the device
    ok &= lmj_decode_interval(sc, T, j, nint, j ? rst[j - 1] : 0u, j + 1 < nint ? rst[j] : sc.len, coef, dcdiff);
  return ok;
}

// DC prediction: per-component running sums of the differences, restarted at
// each restart interval, narrowed to int16 as Decoder::decode_block does.
inline void lmj_dc_host(const LmjScan& sc, int16_t* coef, const int32_t* dcdiff) {
  int32_t pred[3] = {0, 0, 0};
  for (uint32_t blk = 0; blk < sc.nblk; ++blk) {
    if (lmj_dc_reset(sc, blk)) pred[0] = pred[1] = pred[2] = 0;
    const int c = (int)lmj_comp_of(sc, blk % sc.bpm);
    if (c >= 2) continue;
    pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)dcdiff[blk]);
    coef[(uint64_t)blk * 64] = (int16_t)pred[c];
  }
}
#endif  // !__HIP_DEVICE_COMPILE__

#endif  // LM_JPEG_SCAN_H
