// train_core_check.cpp — csrc/lm_train_core.h on the host as a stand-alone
// program (built with -fsanitize=address,undefined by tests/test_train.py):
// random and degenerate sample sets (N = 1, D = 1, all-zero and all-255
// patches, one class, padded rows) through the objective, the Hessian
// product and the line search, with the properties that hold whatever the
// data: the gradient matches central differences of F, v . H v >= |v|^2, the
// Hessian product is linear and symmetric, the line search's step lowers F by
// what it reports, and nothing reads outside its buffers (each buffer is
// allocated at its exact size).  Exits 0 and prints "<n> cases, 0 failures".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lm_train_core.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static double unif() { return (double)rnd() / 4294967296.0 - 0.5; }

static int failures = 0;
static void expect(bool ok, int c, const char* what, double a, double b) {
  if (!ok && failures++ < 10) printf("case %d: %s: %.17g vs %.17g\n", c, what, a, b);
}

int main(int argc, char** argv) {
  const int cases = argc > 1 ? atoi(argv[1]) : 200;
  if (argc > 2) g_state ^= strtoull(argv[2], nullptr, 10);
  for (int c = 0; c < cases; ++c) {
    const int kind = c % 8;
    const int64_t N = kind == 0 ? 1 : 1 + rnd() % 40;
    const int D = kind == 1 ? 1 : 1 + (int)(rnd() % 50);
    const bool padded = rnd() % 2;
    const int64_t pitch = padded ? lmt_pitch(D) : D;
    std::vector<uint8_t> X((size_t)(N * pitch), 0);
    std::vector<int8_t> y((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
      y[(size_t)i] = kind == 4 ? 1 : (rnd() % 2 ? 1 : -1);  // kind 4: one class
      for (int j = 0; j < D; ++j)
        X[(size_t)(i * pitch + j)] = kind == 2 ? 0 : kind == 3 ? 255 : (uint8_t)(rnd() & 255);
    }
    const double cp = kind == 5 ? 10.0 : 0.25 + 4 * (unif() + 0.5), cn = 0.25 + 4 * (unif() + 0.5);
    std::vector<double> wb((size_t)D + 1), g((size_t)D + 1), z((size_t)N), a((size_t)N), t((size_t)N);
    const double scale = c % 3 == 0 ? 0.0 : 4.0 / std::sqrt((double)D);
    for (auto& v : wb) v = scale * unif();
    double F;
    const int64_t na = lmt_host_objective(X.data(), pitch, y.data(), N, D, cp, cn, wb.data(), z.data(), a.data(),
                                          t.data(), &F, g.data());
    expect(na >= 0 && na <= N, c, "active count", (double)na, (double)N);
    expect(F >= 0.0 && std::isfinite(F), c, "objective", F, 0.0);
    // the gradient against central differences (F is C^1, piecewise quadratic)
    for (int j = 0; j <= D; j += 1 + D / 6) {
      std::vector<double> w2(wb), z2((size_t)N), a2((size_t)N), t2((size_t)N), g2((size_t)D + 1);
      const double h = 1e-5;
      double Fp, Fm;
      w2[(size_t)j] = wb[(size_t)j] + h;
      lmt_host_objective(X.data(), pitch, y.data(), N, D, cp, cn, w2.data(), z2.data(), a2.data(), t2.data(), &Fp,
                         g2.data());
      w2[(size_t)j] = wb[(size_t)j] - h;
      lmt_host_objective(X.data(), pitch, y.data(), N, D, cp, cn, w2.data(), z2.data(), a2.data(), t2.data(), &Fm,
                         g2.data());
      const double fd = (Fp - Fm) / (2 * h);
      // |F''| <= 1 + 2 N max(c): the difference quotient is within h times that
      // (where it crosses a kink), plus the rounding of F over 2 h
      const double tol = h * (1 + 2 * (double)N * (cp > cn ? cp : cn)) + 1e-8 * (1 + std::fabs(F));
      expect(std::fabs(fd - g[(size_t)j]) <= tol, c, "gradient vs central difference", fd, g[(size_t)j]);
    }
    // the Hessian product: v.Hv >= |v|^2, symmetric, linear
    std::vector<double> v((size_t)D + 1), w((size_t)D + 1), Hv((size_t)D + 1), Hw((size_t)D + 1), u((size_t)N);
    for (auto& e : v) e = unif();
    for (auto& e : w) e = unif();
    lmt_host_hessvec(X.data(), pitch, N, D, a.data(), v.data(), u.data(), Hv.data());
    lmt_host_hessvec(X.data(), pitch, N, D, a.data(), w.data(), u.data(), Hw.data());
    double vHv = 0, vv = 0, wHv = 0, vHw = 0, mag = 0;
    for (int j = 0; j <= D; ++j) {
      vHv += v[(size_t)j] * Hv[(size_t)j];
      vv += v[(size_t)j] * v[(size_t)j];
      wHv += w[(size_t)j] * Hv[(size_t)j];
      vHw += v[(size_t)j] * Hw[(size_t)j];
      mag += std::fabs(w[(size_t)j] * Hv[(size_t)j]) + std::fabs(v[(size_t)j] * Hw[(size_t)j]);
    }
    expect(vHv >= vv * (1 - 1e-12), c, "v.Hv >= |v|^2", vHv, vv);
    expect(std::fabs(wHv - vHw) <= 1e-10 * (1 + mag) * (double)(N + D), c, "symmetry", wHv, vHw);
    // the line search along -g lowers F by what it reports
    std::vector<double> d((size_t)D + 1), xd((size_t)N);
    double wd = 0, dd = 0, gd = 0;
    for (int j = 0; j <= D; ++j) {
      d[(size_t)j] = -g[(size_t)j];
      wd += wb[(size_t)j] * d[(size_t)j];
      dd += d[(size_t)j] * d[(size_t)j];
      gd += g[(size_t)j] * d[(size_t)j];
    }
    // xd = X~ d: the margins of d as a model
    lmt_host_margins(X.data(), pitch, N, D, d.data(), xd.data());
    double dF;
    const int k = lmt_host_linesearch(y.data(), z.data(), xd.data(), N, cp, cn, wd, dd, gd, &dF);
    if (dd > 1e-20) {
      expect(k >= 0, c, "a step along -g exists", (double)k, 0);
      if (k >= 0) {
        const double lambda = std::ldexp(1.0, -k);
        std::vector<double> w2((size_t)D + 1), z2((size_t)N), a2((size_t)N), t2((size_t)N), g2((size_t)D + 1);
        for (int j = 0; j <= D; ++j) w2[(size_t)j] = wb[(size_t)j] + lambda * d[(size_t)j];
        double F2;
        lmt_host_objective(X.data(), pitch, y.data(), N, D, cp, cn, w2.data(), z2.data(), a2.data(), t2.data(), &F2,
                           g2.data());
        expect(dF <= LMT_ARMIJO * lambda * gd, c, "Armijo", dF, LMT_ARMIJO * lambda * gd);
        expect(std::fabs((F2 - F) - dF) <= 1e-9 * (1 + std::fabs(F) + std::fabs(F2)), c, "reported change of F", F2 - F,
               dF);
      }
    }
  }
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
