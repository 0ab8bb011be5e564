// bkg_core_check.cpp — csrc/lm_bkg_core.h on the host against a brute-force
// sort, as a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_bkg.py): random small cases of every shape of input the kernels
// see — tight and padded pitch, several pushes, constant / two-valued / ramp /
// random pixels, every permille edge.  Exits 0 and prints "<n> cases, 0
// failures" when every pixel agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lm_bkg_core.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int main(int argc, char** argv) {
  const int cases = argc > 1 ? atoi(argv[1]) : 300;
  if (argc > 2) g_state ^= strtoull(argv[2], nullptr, 10);
  int failures = 0;
  for (int c = 0; c < cases; ++c) {
    const size_t npix = 1 + rnd() % 41;
    const int K = 1 + (int)(rnd() % (c % 10 == 0 ? 700 : 40));
    const int64_t pitch = (int64_t)npix + (rnd() % 3 ? 0 : rnd() % 7);
    std::vector<uint8_t> frames((size_t)pitch * K, 0xEE);
    for (size_t p = 0; p < npix; ++p) {
      const uint32_t kind = rnd() % 6, a = rnd() & 255, b = rnd() & 255;
      for (int i = 0; i < K; ++i) {
        uint32_t v;
        switch (kind) {
          case 0: v = a; break;                               // constant
          case 1: v = i % 2 ? 255 : 0; break;                 // alternating extremes
          case 2: v = i < K / 2 ? a : b; break;               // two values, a tie at even K
          case 3: v = (a + (uint32_t)i) & 255; break;         // a new bin every frame
          case 4: v = 126 + rnd() % 5; break;                 // within +-2 of 128
          default: v = rnd() & 255; break;
        }
        frames[(size_t)i * pitch + p] = (uint8_t)v;
      }
    }
    std::vector<lmb_count> hist(npix * LMB_BINS, 0);
    for (int done = 0; done < K;) {  // several pushes
      const int n = std::min(K - done, 1 + (int)(rnd() % 9));
      lmb_host_accumulate(hist.data(), frames.data() + (size_t)done * pitch, pitch, n, npix);
      done += n;
    }
    const int permilles[] = {0, 250, 500, 999, 1000, (int)(rnd() % 1001)};
    for (int pm : permilles) {
      std::vector<uint8_t> got(npix);
      lmb_host_select(hist.data(), npix, pm, K, got.data());
      const int64_t rank = ((int64_t)pm * (K - 1)) / 1000;
      for (size_t p = 0; p < npix; ++p) {
        std::vector<uint8_t> col((size_t)K);
        for (int i = 0; i < K; ++i) col[(size_t)i] = frames[(size_t)i * pitch + p];
        std::sort(col.begin(), col.end());
        if (got[p] != col[(size_t)rank]) {
          if (failures++ < 5)
            printf("case %d pixel %zu permille %d K %d: got %d want %d\n", c, p, pm, K, got[p], col[(size_t)rank]);
        }
      }
    }
  }
  // a counter at the cap: LMB_MAX_SAMPLES equal samples in runs, no wrap
  {
    std::vector<lmb_count> h(LMB_BINS, 0);
    std::vector<uint8_t> f(4096, 7);
    int64_t left = LMB_MAX_SAMPLES;
    while (left > 0) {
      const int n = (int)std::min<int64_t>(left, 4096);
      lmb_host_accumulate(h.data(), f.data(), 1, n, 1);
      left -= n;
    }
    uint8_t v = 0;
    lmb_host_select(h.data(), 1, 1000, LMB_MAX_SAMPLES, &v);
    if (h[7] != LMB_MAX_SAMPLES || v != 7) {
      ++failures;
      printf("cap: counter %u value %d\n", (unsigned)h[7], v);
    }
  }
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
