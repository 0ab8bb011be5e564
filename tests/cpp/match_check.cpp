// match_check.cpp — csrc/lm_match_core.h on the host, stand-alone (its own
// main; tests/test_match.py builds it plainly and with
// -fsanitize=address,undefined).
//
//   match_check                 seeded images and reference CDFs through the core, each compared with a brute-force
//                               statement of locomouse_match.h's definition; prints one summary line, exits 1 on a
//                               difference
//   match_check dump IN OUT     IN: int32 rows, cols, pitch; rows * pitch bytes; 256 floats (a reference CDF).
//                               OUT: 256 uint32 (histogram), 256 floats (CDF), 256 bytes (table), int32 (entries the
//                               second loop decided) -- for the comparison with tests/match_ref.py
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lm_match_core.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the definition once more, the slow way: a count per grey level, a sum per
// CDF entry written out as the chain it is, and the table with explicit
// searches over vectors
struct Brute {
  std::vector<uint32_t> h;
  std::vector<float> c;
  std::vector<uint8_t> T;
  int fallback = 0;
};
Brute brute(const std::vector<uint8_t>& img, int rows, int cols, int pitch, const std::vector<float>& ref) {
  Brute B;
  B.h.assign(256, 0u);
  for (int v = 0; v < 256; ++v)
    for (int r = 0; r < rows; ++r) B.h[v] += (uint32_t)std::count(img.begin() + (size_t)r * pitch, img.begin() + (size_t)r * pitch + cols, (uint8_t)v);
  const double n = (double)rows * (double)cols;
  const float alpha = (float)(1.0 / n);
  B.c.assign(256, 0.f);
  for (int i = 0; i < 256; ++i) {
    volatile float p = (float)B.h[i] * alpha;
    volatile float s = i ? B.c[i - 1] + p : p;
    B.c[i] = s;
  }
  B.T.assign(256, 0);
  int cur = 0;
  for (int i = 0; i < 256; ++i) {
    const float ci = B.c[i];
    auto it = std::find_if(ref.begin() + cur, ref.end(), [&](float r) { return r >= ci; });
    if (it != ref.end()) {
      cur = (int)(it - ref.begin());
    } else {
      float best = 1.0f;
      int at = cur;
      for (int j = cur; j < 256; ++j) {
        volatile float d = ci - ref[j];
        if (d < best) {
          best = d;
          at = j;
        }
      }
      cur = at;
      ++B.fallback;
    }
    B.T[i] = (uint8_t)cur;
  }
  return B;
}

struct Core {
  uint32_t h[256];
  float c[256];
  uint8_t T[256];
  int fallback;
};
Core core(const std::vector<uint8_t>& img, int rows, int cols, int pitch, const std::vector<float>& ref) {
  Core C;
  lm_match_hist(img.data(), rows, cols, pitch, C.h);
  lm_match_cdf_of(C.h, lm_match_scale((int64_t)rows * cols), C.c);
  C.fallback = lm_match_table(C.c, ref.data(), C.T);
  return C;
}

std::vector<float> make_ref(int kind) {
  std::vector<float> r(256);
  switch (kind) {
    case 0: {  // a random image's CDF
      std::vector<uint8_t> im(61 * 53);
      for (auto& v : im) v = (uint8_t)(rnd() % (1 + rnd() % 256));
      uint32_t h[256];
      lm_match_hist(im.data(), 61, 53, 53, h);
      lm_match_cdf_of(h, lm_match_scale(61 * 53), r.data());
      break;
    }
    case 1:  // ends below 1: the second loop runs
      for (int i = 0; i < 256; ++i) r[i] = 0.9f * (float)(i + 1) / 256.0f;
      break;
    case 2:  // long plateaus
      for (int i = 0; i < 256; ++i) r[i] = (float)(i / 64 + 1) * 0.25f;
      break;
    default:  // all zero: every entry above c = 0 falls through
      for (int i = 0; i < 256; ++i) r[i] = 0.f;
  }
  return r;
}

int self_check() {
  int cases = 0, failures = 0, fallback_cases = 0, first_branch_cases = 0;
  const int shapes[][2] = {{1, 1}, {7, 13}, {31, 33}, {64, 64}, {97, 1}, {1, 257}, {41, 61}};
  for (int rep = 0; rep < 40; ++rep)
    for (const auto& sh : shapes)
      for (int kind = 0; kind < 4; ++kind) {
        const int rows = sh[0], cols = sh[1], pitch = cols + (int)(rnd() % 5);
        std::vector<uint8_t> img((size_t)rows * pitch);
        const int mode = (int)(rnd() % 4);
        const uint8_t one = (uint8_t)rnd();
        for (auto& v : img) v = mode == 0 ? one : mode == 1 ? (uint8_t)(rnd() % 3 * 100) : (uint8_t)rnd();
        const std::vector<float> ref = make_ref(kind);
        if (lm_match_cdf_bad(ref.data())) ++failures;
        const Core C = core(img, rows, cols, pitch, ref);
        const Brute B = brute(img, rows, cols, pitch, ref);
        ++cases;
        const bool same = std::equal(B.h.begin(), B.h.end(), C.h) && std::memcmp(B.c.data(), C.c, sizeof(C.c)) == 0 &&
                          std::equal(B.T.begin(), B.T.end(), C.T) && B.fallback == C.fallback;
        if (!same) {
          ++failures;
          std::printf("case %d (%d x %d, ref %d) differs\n", cases, rows, cols, kind);
        }
        fallback_cases += C.fallback > 0;
        first_branch_cases += C.fallback < 256;
      }
  // the validation's three refusals, and NaN / infinity
  std::vector<float> bad = make_ref(1);
  bad[10] = -1e-3f;
  failures += lm_match_cdf_bad(bad.data()) == nullptr;
  bad = make_ref(1);
  bad[200] = bad[199] - 1e-3f;
  failures += lm_match_cdf_bad(bad.data()) == nullptr;
  bad = make_ref(1);
  bad[255] = std::numeric_limits<float>::infinity();
  failures += lm_match_cdf_bad(bad.data()) == nullptr;
  bad[255] = std::numeric_limits<float>::quiet_NaN();
  failures += lm_match_cdf_bad(bad.data()) == nullptr;
  std::printf("%d cases, fallback in %d, first branch in %d, %d failures\n", cases, fallback_cases, first_branch_cases,
              failures);
  return failures || !fallback_cases || !first_branch_cases ? 1 : 0;
}

int dump(const char* in, const char* out) {
  std::FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  int32_t hd[3];
  if (std::fread(hd, sizeof(hd), 1, f) != 1 || hd[0] <= 0 || hd[1] <= 0 || hd[2] < hd[1]) return 2;
  std::vector<uint8_t> img((size_t)hd[0] * hd[2]);
  std::vector<float> ref(256);
  if (std::fread(img.data(), 1, img.size(), f) != img.size() || std::fread(ref.data(), 4, 256, f) != 256) return 2;
  std::fclose(f);
  const Core C = core(img, hd[0], hd[1], hd[2], ref);
  f = std::fopen(out, "wb");
  if (!f) return 2;
  const int32_t fb = C.fallback;
  const bool ok = std::fwrite(C.h, 4, 256, f) == 256 && std::fwrite(C.c, 4, 256, f) == 256 &&
                  std::fwrite(C.T, 1, 256, f) == 256 && std::fwrite(&fb, 4, 1, f) == 1;
  std::fclose(f);
  return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "dump")) return dump(argv[2], argv[3]);
  if (argc != 1) {
    std::fprintf(stderr, "usage: match_check [dump IN OUT]\n");
    return 2;
  }
  return self_check();
}
