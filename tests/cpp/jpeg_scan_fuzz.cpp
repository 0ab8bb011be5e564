// jpeg_scan_fuzz.cpp — stand-alone check of the device decoder's host-runnable
// code (csrc/lm_jpeg_scan.h, lm_jpeg_hdr.h) under the host sanitizers:
//
//   jpeg_scan_fuzz <seed> <variants> file.jpg ...
//
// Every file, then copies of it truncated or with bytes overwritten at seeded
// positions, goes through the header parse, the lane-by-lane subsequence scan
// (several subsequence sizes and chunk widths), DC sums, IDCT and channel 0.
// Checked: the given files decode to the host decoder's bytes; a damaged copy
// either ends in a status or — when the scan raised no error — also equals the
// host decoder's bytes; sync rounds never exceed the subsequences.  Memory
// errors and undefined behaviour are the sanitizers' to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Jpeg.hpp"
#include "lm_jpeg_hdr.h"
#include "lm_jpeg_scan.h"

namespace {

uint64_t g_rng = 1;
uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

struct Result {
  int cls = 2;  // 0 decoded, 1 needs host, 2 rejected
  std::vector<uint8_t> px;
  int W = 0, H = 0;
};

int g_fail = 0;
void fail(const char* what, const char* file, int variant) {
  std::fprintf(stderr, "FAIL %s: %s (variant %d)\n", what, file, variant);
  ++g_fail;
}

Result lanes_decode(const std::vector<uint8_t>& j, int subseq, int lanes, const char* file, int variant) {
  Result R;
  lmj::Header h;
  lmj::parse(j.data(), j.size(), h);
  R.cls = (int)h.cls;
  if (h.cls != lmj::kInScope) return R;
  if ((int64_t)h.W * h.H > (1 << 22)) {  // a corrupted size field: keep the run small
    R.cls = 1;
    return R;
  }
  LmjTableSet T;
  lmj::make_tables(h, T);
  LmjScan sc = lmj::make_scan(h, (uint32_t)subseq);
  // an exact-size copy, so that a read past the scan is a heap overflow the sanitizer sees
  std::vector<uint8_t> scan(j.begin() + (long)h.scan_off, j.begin() + (long)(h.scan_off + h.scan_len));
  sc.d = scan.data();
  std::vector<int16_t> coef((size_t)sc.nblk * 64);
  std::vector<int32_t> dcd(sc.nblk);
  LmjScanStats st;
  const uint32_t e = lmj_scan_frame_host(sc, T, lanes, coef.data(), dcd.data(), &st);
  if (st.rounds > st.subsequences || st.max_rounds > (uint32_t)lanes) fail("sync rounds exceed the subsequences", file, variant);
  if (e) {
    R.cls = 1;
    return R;
  }
  lmj_dc_host(sc, coef.data(), dcd.data());
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
  R.W = h.W;
  R.H = h.H;
  R.px.resize((size_t)h.W * h.H);
  for (int y = 0; y < h.H; ++y)
    for (int x = 0; x < h.W; ++x)
      R.px[(size_t)y * h.W + x] = lmj_channel0(py.data(), pc.data(), P, h.nc, sc.hx, sc.vx, x, y);
  return R;
}

void check(const std::vector<uint8_t>& j, bool pristine, const char* file, int variant) {
  {
    lmj::Header h;
    lmj::parse(j.data(), j.size(), h);
    if ((int64_t)h.W * h.H > (1 << 22)) return;  // a corrupted size field: keep the run small
  }
  int rows = 0, cols = 0;
  std::vector<uint8_t> want;
  std::string why;
  const bool host_ok = locomouse::decode_jpeg_channel0(j.data(), j.size(), rows, cols, want, &why);
  const int cfg[4][2] = {{LMJ_SUBSEQ_MIN, LMJ_LANES}, {LMJ_SUBSEQ_DEFAULT, LMJ_LANES}, {7, 3}, {1 << 20, 1}};
  for (const auto& c : cfg) {
    const Result R = lanes_decode(j, c[0], c[1], file, variant);
    if (pristine && R.cls != 0) fail("a clean stream was not decoded", file, variant);
    if (R.cls == 2 && host_ok) fail("rejected a stream the host decoder accepts", file, variant);
    if (R.cls == 0) {
      if (!host_ok) fail("decoded a stream the host decoder rejects", file, variant);
      else if (R.W != cols || R.H != rows || R.px != want) fail("pixels differ from the host decoder's", file, variant);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s <seed> <variants> file.jpg ...\n", argv[0]);
    return 2;
  }
  g_rng = std::strtoull(argv[1], nullptr, 10) | 1;
  const int variants = std::atoi(argv[2]);
  int streams = 0, damaged = 0;
  for (int a = 3; a < argc; ++a) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> j;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) j.insert(j.end(), buf, buf + n);
    std::fclose(f);
    if (j.size() < 4) continue;
    check(j, true, argv[a], -1);
    ++streams;
    {  // restart markers the interval asks for but the scan lacks: byte edits do not construct these
      lmj::Header h;
      lmj::parse(j.data(), j.size(), h);
      if (h.cls == lmj::kInScope && h.restart == 0) {  // a DRI segment in front of SOS, no RSTn in the scan
        size_t sos = 0;  // the files are encoder output: segment after segment from byte 2
        for (size_t k = 2; k + 3 < h.scan_off; k += 2 + (size_t)((j[k + 2] << 8) | j[k + 3]))
          if (j[k + 1] == 0xDA) sos = k;
        for (int interval : {1, 3, 1000}) {
          if (!sos) break;
          std::vector<uint8_t> d(j.begin(), j.begin() + (long)sos);
          const uint8_t dri[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(interval >> 8), (uint8_t)(interval & 255)};
          d.insert(d.end(), dri, dri + 6);
          d.insert(d.end(), j.begin() + (long)sos, j.end());
          check(d, false, argv[a], -2);
          ++damaged;
        }
      } else if (h.cls == lmj::kInScope) {  // the last, then the first RSTn taken out
        for (int which = 0; which < 2; ++which) {
          size_t at = 0;
          for (size_t k = h.scan_off; k + 1 < h.scan_off + h.scan_len; ++k)
            if (j[k] == 0xFF && j[k + 1] >= 0xD0 && j[k + 1] <= 0xD7) {
              at = k;
              if (which) break;
            }
          if (!at) continue;
          std::vector<uint8_t> d = j;
          d.erase(d.begin() + (long)at, d.begin() + (long)at + 2);
          check(d, false, argv[a], -3);
          ++damaged;
        }
      }
    }
    for (int v = 0; v < variants; ++v) {
      std::vector<uint8_t> d = j;
      switch (v % 4) {
        case 0:  // truncated
          d.resize(2 + rnd() % (d.size() - 2));
          break;
        case 1:  // truncated, EOI put back
          d.resize(2 + rnd() % (d.size() - 2));
          d.push_back(0xFF);
          d.push_back(0xD9);
          break;
        case 2:  // a few bytes overwritten, anywhere
          for (int k = 0, m = 1 + (int)(rnd() % 4); k < m; ++k) d[rnd() % d.size()] = (uint8_t)rnd();
          break;
        default:  // bytes overwritten in the second half (mostly the scan), FF-heavy
          for (int k = 0, m = 1 + (int)(rnd() % 3); k < m; ++k)
            d[d.size() / 2 + rnd() % (d.size() - d.size() / 2)] = (rnd() & 1) ? 0xFF : (uint8_t)(0xD0 + rnd() % 16);
          break;
      }
      check(d, false, argv[a], v);
      ++damaged;
    }
  }
  std::printf("%d streams, %d damaged copies, %d failures\n", streams, damaged, g_fail);
  return g_fail ? 1 : 0;
}
