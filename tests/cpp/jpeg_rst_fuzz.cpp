// jpeg_rst_fuzz.cpp — stand-alone check of the device decoder's interval path
// as the host runs it (csrc/lm_jpeg_scan.h: lmj_scan_intervals_host and the
// hand-over to lmj_scan_frame_host) under the host sanitizers:
//
//   jpeg_rst_fuzz <seed> <variants> file.jpg ...
//
// Every file (restart-marker streams), then seeded damaged copies of it:
// truncated, bytes overwritten, a marker taken out, doubled, renumbered or put
// where none belongs.  Checked: the interval schedule with its hand-over gives
// the class, the coefficients and the DC differences of the subsequence
// schedule alone, for every copy; a clean restart stream is finished by the
// interval path itself.  Memory errors and undefined behaviour are the
// sanitizers' to report: the scan is an exact-size copy, so a read past it is
// a heap overflow they see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_jpeg_hdr.h"
#include "lm_jpeg_scan.h"

namespace {

uint64_t g_rng = 1;
uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

int g_fail = 0, g_interval = 0, g_handed = 0;
void fail(const char* what, const char* file, int variant) {
  std::fprintf(stderr, "FAIL %s: %s (variant %d)\n", what, file, variant);
  ++g_fail;
}

void check(const std::vector<uint8_t>& j, bool pristine, const char* file, int variant) {
  lmj::Header h;
  std::vector<uint32_t> rst;
  lmj::parse(j.data(), j.size(), h, &rst);
  if (h.cls != lmj::kInScope) {
    if (pristine) fail("a clean stream is out of scope", file, variant);
    return;
  }
  if ((int64_t)h.W * h.H > (1 << 22)) return;  // a corrupted size field: keep the run small
  LmjTableSet T;
  lmj::make_tables(h, T);
  LmjScan sc = lmj::make_scan(h, LMJ_SUBSEQ_DEFAULT);
  std::vector<uint8_t> scan(j.begin() + (long)h.scan_off, j.begin() + (long)(h.scan_off + h.scan_len));
  sc.d = scan.data();
  for (uint32_t off : rst)
    if (off < 2 || off > sc.len) fail("a marker index entry outside the scan", file, variant);
  std::vector<int16_t> coef((size_t)sc.nblk * 64), coef2((size_t)sc.nblk * 64);
  std::vector<int32_t> dcd(sc.nblk), dcd2(sc.nblk);
  const uint32_t want = lmj_scan_frame_host(sc, T, LMJ_LANES, coef2.data(), dcd2.data(), nullptr);
  const bool done = lmj_scan_intervals_host(sc, T, rst.data(), (uint32_t)rst.size(), coef.data(), dcd.data());
  uint32_t e = 0;
  if (!done) e = lmj_scan_frame_host(sc, T, LMJ_LANES, coef.data(), dcd.data(), nullptr);
  ++(done ? g_interval : g_handed);
  if (pristine && !(done && e == 0)) fail("the interval path did not finish a clean restart stream", file, variant);
  if ((e != 0) != (want != 0)) fail("the class differs from the subsequence path's", file, variant);
  if (done && want) fail("the interval path finished a frame the subsequence path refuses", file, variant);
  if (!want && (coef != coef2 || dcd != dcd2)) fail("coefficients differ from the subsequence path's", file, variant);
}

// The k-th restart marker of the scan (its FF), or 0.
size_t marker_at(const std::vector<uint8_t>& j, const lmj::Header& h, uint32_t k) {
  uint32_t seen = 0;
  for (size_t i = h.scan_off; i + 1 < h.scan_off + h.scan_len; ++i)
    if (j[i] == 0xFF && j[i + 1] >= 0xD0 && j[i + 1] <= 0xD7 && seen++ == k) return i;
  return 0;
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
    lmj::Header h;
    std::vector<uint32_t> rst;
    lmj::parse(j.data(), j.size(), h, &rst);
    const uint32_t nm = (uint32_t)rst.size();
    for (int v = 0; v < variants; ++v) {
      std::vector<uint8_t> d = j;
      const size_t m = nm ? marker_at(j, h, rnd() % nm) : 0;
      switch (v % 8) {
        case 0:  // truncated
          d.resize(2 + rnd() % (d.size() - 2));
          break;
        case 1:  // truncated inside the scan, EOI put back
          d.resize(h.scan_off + rnd() % (h.scan_len + 1));
          d.push_back(0xFF);
          d.push_back(0xD9);
          break;
        case 2:  // a few bytes of the scan overwritten
          for (int k = 0, c = 1 + (int)(rnd() % 4); k < c; ++k) d[h.scan_off + rnd() % h.scan_len] = (uint8_t)rnd();
          break;
        case 3:  // bytes of the scan overwritten, FF- and marker-heavy
          for (int k = 0, c = 1 + (int)(rnd() % 3); k < c; ++k)
            d[h.scan_off + rnd() % h.scan_len] = (rnd() & 1) ? 0xFF : (uint8_t)(0xD0 + rnd() % 16);
          break;
        case 4:  // a marker taken out
          if (m) d.erase(d.begin() + (long)m, d.begin() + (long)m + 2);
          break;
        case 5:  // a marker doubled
          if (m) d.insert(d.begin() + (long)m, j.begin() + (long)m, j.begin() + (long)m + 2);
          break;
        case 6:  // a marker renumbered
          if (m) d[m + 1] = (uint8_t)(0xD0 + rnd() % 8);
          break;
        default:  // a marker where none belongs (the count stays right when another is taken out)
        {
          const size_t at = h.scan_off + rnd() % h.scan_len;
          const uint8_t mk[2] = {0xFF, (uint8_t)(0xD0 + rnd() % 8)};
          d.insert(d.begin() + (long)at, mk, mk + 2);
          if (m && (rnd() & 1)) {
            const size_t mm = m >= at ? m + 2 : m;
            d.erase(d.begin() + (long)mm, d.begin() + (long)mm + 2);
          }
          break;
        }
      }
      check(d, false, argv[a], v);
      ++damaged;
    }
  }
  std::printf("%d streams, %d damaged copies, %d finished by the interval path, %d handed over, %d failures\n", streams,
              damaged, g_interval, g_handed, g_fail);
  return g_fail ? 1 : 0;
}
