// f16_plan_check — the plan of k_corr_f16 (locomouse_cpp_amd/csrc/
// lm_corr_f16.h) on the host, for every chunk count NCH = 2..10:
//  * f16_nch / f16_cols of every detector width 1..130,
//  * every LDS address the kernel forms (the A fragments' 16-byte reads, the
//    fill's 16-byte stores, the point detectors' mask reads) inside the window
//    and aligned, for every wave, lane, A step and detector size,
//  * the acceptance cap of the runtime (160 KiB of dynamic LDS) against the
//    compute unit's LDS with the kernel's static variables in front,
//  * an integer emulation of one workgroup: the B fragments of
//    f16_bfrag_weight and the A fragments at the kernel's addresses, combined
//    with the 32x32x16 MFMA's operand and accumulator lane maps and the
//    kernel's pairing (tile 0: A_m x B_m, m < NCH; tile 1: A_m x B_(m-2),
//    m >= 2), against the direct sum  sum w[i][j] I[y + i][x + j]  of every
//    one of the 128 x 64 outputs.  This restates the kernel's indexing (it
//    does not run the kernel): it pins the host's fragment layout and the
//    tile-1 shift identity for every class.
// Prints one summary line; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <set>
#include <vector>

#include "lm_corr_f16.h"

namespace {

constexpr size_t kLdsCap = 160 * 1024;    // lm_runtime.hip kF16LdsMax (validate)
constexpr size_t kLdsUnit = 160 * 1024;   // LDS of a gfx950 compute unit
constexpr size_t kStaticLds = 16;         // k_corr_f16's s_cnt, s_base, rounded to the window's 16-byte alignment

long g_checks = 0, g_failures = 0;
void expect(bool ok, const char* what, long a = 0, long b = 0, long c = 0) {
  ++g_checks;
  if (!ok && g_failures++ < 20) fprintf(stderr, "FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
}

int kw_min(int nch) { return 16 * nch - 46 > 1 ? 16 * nch - 46 : 1; }
int kw_max(int nch) { return 16 * nch - 31; }

// halfs from the window's start of the A fragment of wave (wx, wy), lane
// (r, h), window row 32 wy + r + i, A step m (k_corr_f16: arow, load_a)
long a_addr(int STR, int wx, int wy, int r, int h, int i, int m) {
  return (long)(32 * wy + r + i) * STR + 64 * wx + 8 * h + 16 * m;
}

void check_widths() {
  for (int kw = 1; kw <= 130; ++kw) {
    const int nch = f16_nch(kw);
    expect(kw <= 129 ? (nch >= 2 && nch <= LM_F16_MAX_NCH) : nch == LM_F16_MAX_NCH + 1, "f16_nch range", kw, nch);
    expect(16 * (nch - 1) < kw + 31 && kw + 31 <= 16 * nch, "f16_nch is the least chunk count", kw, nch);
    expect(f16_cols(nch) >= LM_F16_TW + kw - 1, "f16_cols holds the tile's window", kw, nch);
    if (kw <= 129) expect(kw >= kw_min(nch) && kw <= kw_max(nch), "class bounds", kw, nch);
  }
}

// largest detector height validate accepts at this chunk count
int kh_cap(int nch) {
  int kh = 1;
  while (f16_lds_bytes(nch, kh + 1) <= kLdsCap) ++kh;
  return kh;
}

void check_addresses(int nch) {
  const int cols = f16_cols(nch), STR = f16_stride(cols);
  expect(STR % 16 == 8, "row stride == 8 (mod 16) halfs", nch, STR);
  expect(STR >= cols, "row stride holds the columns", nch, STR);
  // the fill: (cols + 7) / 8 16-byte stores per row, the last one inside the stride
  const int ng = (cols + 7) >> 3;
  expect(8 * (ng - 1) + 8 <= STR, "the fill's last store ends inside the stride", nch, ng, STR);
  expect(8 * ng >= cols, "the fill covers the columns", nch, ng);
  const int khs[] = {1, 2, 3, 4, 5, 7, 16, 64, kh_cap(nch)};
  for (int kh : khs) {
    const int rows = LM_F16_TH + kh - 1;
    for (int wx = 0; wx < 2; ++wx)
      for (int wy = 0; wy < 2; ++wy)
        for (int h = 0; h < 2; ++h)
          for (int r = 0; r < 32; ++r) {
            // A fragments: 8 halfs at steps m < nch + 2, detector rows i < kh
            for (int m = 0; m < nch + 2; ++m)
              for (int i : {0, kh - 1}) {
                const long a = a_addr(STR, wx, wy, r, h, i, m);
                const long row = a / STR, col = a % STR;
                expect(a % 8 == 0, "A fragment 16-byte aligned", nch, a);
                expect(row == 32 * wy + r + i && row < rows, "A fragment row inside the window", nch, row, rows);
                expect(col + 8 <= cols, "A fragment ends inside the columns", nch, col, cols);
              }
            // mask reads of a point detector: every width of the class
            for (int kw = kw_min(nch); kw <= kw_max(nch); ++kw)
              for (int t = 0; t < 2; ++t) {
                const int col = 64 * wx + r + 32 * t + kw / 2;
                expect(col < cols, "mask column inside the window", nch, kw, col);
                for (int ly : {0, 31}) {
                  const int row = kh / 2 + 32 * wy + ly;
                  expect(row < rows, "mask row inside the window", nch, kh, row);
                }
              }
          }
  }
}

void check_cap() {
  expect(f16_lds_bytes(10, 247) <= kLdsCap && kLdsCap < f16_lds_bytes(10, 248), "the cap at NCH 10 lies between kh 247 and 248");
  expect(f16_lds_bytes(10, 247) == 163680, "the largest window at NCH 10", (long)f16_lds_bytes(10, 247));
  expect(f16_lds_bytes(10, 64) == 67056, "the 64 x 129 window", (long)f16_lds_bytes(10, 64));
  for (int nch = 2; nch <= LM_F16_MAX_NCH; ++nch) {
    const int kh = kh_cap(nch);
    expect(f16_lds_bytes(nch, kh) <= kLdsCap && f16_lds_bytes(nch, kh + 1) > kLdsCap, "kh_cap", nch, kh);
    expect(f16_lds_bytes(nch, kh) + kStaticLds <= kLdsUnit, "largest accepted window + static LDS fits the unit", nch, kh,
           (long)f16_lds_bytes(nch, kh));
  }
}

struct Stats {
  long by_nch[LM_F16_MAX_NCH + 1] = {0}, by_kh[8] = {0}, workgroups = 0, sums = 0;
} S;

// One workgroup at (nch, kw, kh) in integers.
void emulate(int nch, int kw, int kh, std::mt19937& rng) {
  const int cols = f16_cols(nch), STR = f16_stride(cols), rows = LM_F16_TH + kh - 1;
  // weights: small integers, every tap non-zero at the band's ends (a dropped first or last tap must show)
  std::vector<double> w((size_t)kh * kw);
  for (double& v : w) v = (double)((int)(rng() % 9) - 4);
  for (int i = 0; i < kh; ++i) {
    if (w[(size_t)i * kw] == 0) w[(size_t)i * kw] = 3;
    if (w[(size_t)i * kw + kw - 1] == 0) w[(size_t)i * kw + kw - 1] = -2;
  }
  // the window as the fill leaves it: rows x STR halfs, of which `cols` per row are pixels
  std::vector<int32_t> img((size_t)rows * STR);
  for (int32_t& v : img) v = (int32_t)(rng() % 256);
  // B fragments as f16_fragments lays them out: [i][c][lane][j]
  std::vector<int32_t> bf((size_t)kh * nch * 64 * 8);
  for (int i = 0; i < kh; ++i)
    for (int c = 0; c < nch; ++c)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) bf[(((size_t)i * nch + c) * 64 + l) * 8 + j] = (int32_t)f16_bfrag_weight(w.data(), kw, i, c, l, j);
  long bad = 0;
  for (int wave = 0; wave < LM_F16_WAVES; ++wave) {
    const int wx = wave & 1, wy = wave >> 1;
    // acc[t][lane][reg]
    std::vector<int64_t> acc((size_t)2 * 64 * 16, 0);
    // one v_mfma_f32_32x32x16: operand element j of lane l is k = 8 (l >> 5) + j; the A row and the B column are
    // l & 31; accumulator reg q of lane l is row (q & 3) + 8 (q >> 2) + 4 (l >> 5), column l & 31
    auto mfma = [&](int t, int i, int m, int c) {
      int32_t A[32][16], B[16][32];
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int k = 8 * (l >> 5) + j;
          A[l & 31][k] = img[(size_t)a_addr(STR, wx, wy, l & 31, l >> 5, i, m) + j];
          B[k][l & 31] = bf[(((size_t)i * nch + c) * 64 + l) * 8 + j];
        }
      for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * (l >> 5), col = l & 31;
          int64_t s = 0;
          for (int k = 0; k < 16; ++k) s += (int64_t)A[row][k] * B[k][col];
          acc[((size_t)t * 64 + l) * 16 + q] += s;
        }
    };
    for (int i = 0; i < kh; ++i)
      for (int m = 0; m < nch + 2; ++m) {
        if (m < nch) mfma(0, i, m, m);
        if (m >= 2) mfma(1, i, m, m - 2);
      }
    for (int t = 0; t < 2; ++t)
      for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 16; ++q) {
          const int y = 32 * wy + (q & 3) + 8 * (q >> 2) + 4 * (l >> 5), x = 64 * wx + 32 * t + (l & 31);
          int64_t ref = 0;
          for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) ref += (int64_t)w[(size_t)i * kw + j] * img[(size_t)(y + i) * STR + x + j];
          ++S.sums;
          if (acc[((size_t)t * 64 + l) * 16 + q] != ref) ++bad;
        }
  }
  expect(bad == 0, "emulated workgroup differs from the direct sums", nch, kw, kh);
  ++S.workgroups;
  ++S.by_nch[nch];
  ++S.by_kh[kh];
}

}  // namespace

int main() {
  check_widths();
  check_cap();
  std::mt19937 rng(20241021u);
  for (int nch = 2; nch <= LM_F16_MAX_NCH; ++nch) {
    check_addresses(nch);
    const std::set<int> kws = {kw_min(nch), (kw_min(nch) + kw_max(nch)) / 2, kw_max(nch)};
    for (int kw : kws) {
      expect(f16_nch(kw) == nch, "the width is of its class", nch, kw);
      for (int kh : {1, 2, 3, 4, 5, 7}) emulate(nch, kw, kh, rng);
    }
  }
  printf("nch");
  for (int n = 2; n <= LM_F16_MAX_NCH; ++n) printf(" %d:%ld", n, S.by_nch[n]);
  printf(", kh");
  for (int kh : {1, 2, 3, 4, 5, 7}) printf(" %d:%ld", kh, S.by_kh[kh]);
  printf(", %ld workgroups, %ld sums, %ld checks, %ld failures\n", S.workgroups, S.sums, g_checks, g_failures);
  return g_failures ? 1 : 0;
}
