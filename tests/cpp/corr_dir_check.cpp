// corr_dir_check — the ring correlation's wave directory (locomouse_cpp_amd/
// csrc/lm_corr_dir.h) against the walk it replaces, on the host: for launch
// groups of 1 to 6 listed and unlisted detectors and many sets of list
// counters, every wave g of the grid is located twice, by walking the group's
// detectors in order (lm_corr.hip corr_locate_walk, restated here) and by the
// directory record (lm_cd_record, lm_cd_lookup: what k_corr_dir writes and
// corr_locate_dir reads), and both must give the same detector, segment, place
// in the segment and number of valid sub-tiles, or both nothing.
// Prints one summary line; exit status 1 on any failure.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "lm_corr_dir.h"

namespace {

constexpr int kWavesPerWorkgroup = 4;  // LM_RW_WAVES: the grid is whole workgroups

struct Det {
  bool listed;
  int nt;                    // 80 x 16 tiles per slot
  int32_t cnt[LM_TL_NC];     // listed: tiles per segment
};
struct Group {
  std::vector<Det> det;
  int nslots;
};
struct Where {
  bool found;
  int k, c, w, nvalid;  // detector's place in the group; listed: segment, place, valid sub-tiles; unlisted: c = -1, w = local
  bool operator==(const Where& o) const {
    return found == o.found && (!found || (k == o.k && c == o.c && w == o.w && nvalid == o.nvalid));
  }
};

long g_checks = 0, g_failures = 0;
void fail(const char* what, int g) {
  if (g_failures++ < 20) fprintf(stderr, "FAIL %s at wave %d\n", what, g);
}

// corr_listed_run's arithmetic: the inclusive scan over the 64 counters, the
// first segment whose scan exceeds `local`, the place in it.
Where listed_wave(const Det& D, int k, int local) {
  int P[LM_TL_NC], wv[LM_TL_NC];
  for (int c = 0; c < LM_TL_NC; ++c) {
    wv[c] = lm_cd_seg_waves(D.cnt[c]);
    P[c] = wv[c] + (c ? P[c - 1] : 0);
  }
  int c = 0;
  while (c < LM_TL_NC && !(P[c] > local)) ++c;
  if (c == LM_TL_NC) return Where{false, 0, 0, 0, 0};
  const int w = local - (P[c] - wv[c]);
  return Where{true, k, c, w, std::min((int)LM_RW_NQ, D.cnt[c] - LM_RW_NQ * w)};
}

int det_waves(const Det& D, int nslots) {
  return D.listed ? lm_cd_listed_waves(D.cnt) : lm_cd_unlisted_waves(D.nt, nslots);
}

// the walk: detector by detector, a running base
Where walk(const Group& G, int g) {
  int base = 0;
  for (int k = 0; k < LM_NDET; ++k) {
    if (k >= (int)G.det.size()) return Where{false, 0, 0, 0, 0};
    const Det& D = G.det[k];
    if (D.listed) {
      int cnt = 0;
      for (int c = 0; c < LM_TL_NC; ++c) cnt += (D.cnt[c] + LM_RW_NQ - 1) / LM_RW_NQ;
      if (g < base + cnt) return listed_wave(D, k, g - base);
      base += cnt;
    } else {
      const int cnt = D.nt * G.nslots;
      if (g < base + cnt) return Where{true, k, -1, g - base, LM_RW_NQ};
      base += cnt;
    }
  }
  return Where{false, 0, 0, 0, 0};
}

// by the record
Where by_dir(const Group& G, const LmCorrDirRec& r, int g) {
  int k, local;
  if (!lm_cd_lookup(r, (int)G.det.size(), g, &k, &local)) return Where{false, 0, 0, 0, 0};
  const Det& D = G.det[k];
  if (D.listed) return listed_wave(D, k, local);
  return Where{true, k, -1, local, LM_RW_NQ};
}

struct Stats {
  long groups = 0, waves = 0, empty = 0, full = 0, mixed = 0, by_n[LM_NDET + 1] = {0}, past = 0;
} S;

void check_group(const Group& G) {
  const int n = (int)G.det.size();
  int32_t waves[LM_NDET] = {0};
  int tiles = 0;
  bool any_listed = false, any_unlisted = false;
  for (int k = 0; k < n; ++k) {
    waves[k] = det_waves(G.det[k], G.nslots);
    tiles += G.det[k].nt;
    (G.det[k].listed ? any_listed : any_unlisted) = true;
  }
  const LmCorrDirRec r = lm_cd_record(waves, n);
  const int need = tiles * G.nslots;  // the grid's waves before rounding to workgroups (launch_corr)
  const int grid = (need + kWavesPerWorkgroup - 1) / kWavesPerWorkgroup * kWavesPerWorkgroup;
  ++g_checks;
  if (r.total > need) fail("the group's waves exceed its grid", r.total);
  for (int k = 0; k < LM_NDET; ++k) {
    ++g_checks;
    if (r.end[k] < (k ? r.end[k - 1] : 0) || (k >= n - 1 && r.end[k] != r.total)) fail("record not cumulative", k);
  }
  int seen = 0;
  for (int g = 0; g < grid + 2 * kWavesPerWorkgroup; ++g) {
    const Where a = walk(G, g), b = by_dir(G, r, g);
    ++g_checks;
    if (!(a == b)) fail("walk and directory differ", g);
    ++g_checks;
    if (g >= r.total && (a.found || b.found)) fail("a wave past the total found work", g);
    if (g < r.total && !(a.found && b.found)) fail("a wave below the total found nothing", g);
    if (a.found) {
      ++seen;
      ++g_checks;
      if (a.c >= 0 && (a.nvalid < 1 || a.nvalid > LM_RW_NQ)) fail("nvalid out of range", g);
    } else {
      ++S.past;
    }
  }
  ++g_checks;
  if (seen != r.total) fail("waves with work != total", seen);
  ++S.groups;
  S.waves += grid;
  ++S.by_n[n];
  if (r.total == 0) ++S.empty;
  if (r.total == need && any_listed) ++S.full;  // every tile of the grid has its wave
  if (any_listed && any_unlisted) ++S.mixed;
}

// slots whose tiles segment c holds (k_ingest: slot groups of LM_INGEST_FB)
int seg_slots(int c, int nslots) {
  const int ng = (nslots + LM_INGEST_FB - 1) / LM_INGEST_FB;
  const int y0 = lm_tl_y0(c, ng), y1 = c + 1 < LM_TL_NC ? lm_tl_y0(c + 1, ng) : ng;
  int s = 0;
  for (int y = y0; y < y1 && y < ng; ++y) s += std::min(LM_INGEST_FB, nslots - y * LM_INGEST_FB);
  return s;
}

Det listed(int nt) {
  Det D{};
  D.listed = true;
  D.nt = nt;
  return D;
}
Det unlisted(int nt) {
  Det D{};
  D.listed = false;
  D.nt = nt;
  return D;
}

}  // namespace

int main() {
  // all zero
  for (int n = 1; n <= LM_NDET; ++n) {
    Group G{{}, 9};
    for (int k = 0; k < n; ++k) G.det.push_back(listed(3 + k));
    check_group(G);
  }
  // a single entry in a single segment, in every segment and every detector
  for (int n = 1; n <= LM_NDET; ++n)
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < LM_TL_NC; c += (c < 2 || c > 60) ? 1 : 7) {
        Group G{{}, 512};
        for (int j = 0; j < n; ++j) G.det.push_back(listed(4));
        G.det[k].cnt[c] = 1;
        check_group(G);
      }
  // exact multiples of LM_RW_NQ and one more
  for (int m : {1, 2, 5})
    for (int extra : {0, 1}) {
      Group G{{listed(40), listed(40), listed(40)}, 512};
      for (int k = 0; k < 3; ++k)
        for (int c = 0; c < LM_TL_NC; c += k + 1) G.det[k].cnt[c] = LM_RW_NQ * m + extra;
      check_group(G);
    }
  // every place of every slot listed: the total equals the grid
  for (int nslots : {1, 3, 8, 9, 64, 449, 512, 513})
    for (int n = 1; n <= LM_NDET; ++n) {
      Group G{{}, nslots};
      for (int k = 0; k < n; ++k) {
        Det D = listed(2 + 3 * k);
        for (int c = 0; c < LM_TL_NC; ++c) D.cnt[c] = LM_RW_NQ * D.nt * seg_slots(c, nslots);
        G.det.push_back(D);
      }
      check_group(G);
    }
  // listed and unlisted detectors mixed, groups of 1 to 6, and seeded random counters within each segment's room
  std::mt19937 rng(20240607u);
  for (int it = 0; it < 600; ++it) {
    const int n = 1 + it % LM_NDET;
    const int nslots = std::vector<int>{1, 3, 4, 9, 17, 64, 100, 449}[rng() % 8];
    Group G{{}, nslots};
    for (int k = 0; k < n; ++k) {
      const int nt = 1 + (int)(rng() % 12);
      if (rng() % 3 == 0) {
        G.det.push_back(unlisted(nt));
        continue;
      }
      Det D = listed(nt);
      const int mode = (int)(rng() % 4);  // sparse, dense, a few segments, full
      for (int c = 0; c < LM_TL_NC; ++c) {
        const int room = LM_RW_NQ * nt * seg_slots(c, nslots);
        if (room == 0) continue;
        switch (mode) {
          case 0: D.cnt[c] = (int)(rng() % 5 == 0 ? rng() % (unsigned)std::min(room + 1, 12) : 0); break;
          case 1: D.cnt[c] = (int)(rng() % (unsigned)(room + 1)); break;
          case 2: D.cnt[c] = (int)(rng() % 16 == 0 ? rng() % (unsigned)(room + 1) : 0); break;
          default: D.cnt[c] = room - (int)(rng() % 2); break;
        }
      }
      G.det.push_back(D);
    }
    check_group(G);
  }
  printf("%ld groups, %ld waves, %ld empty, %ld full, %ld mixed, n %ld %ld %ld %ld %ld %ld, %ld past, %ld checks, %ld failures\n",
         S.groups, S.waves, S.empty, S.full, S.mixed, S.by_n[1], S.by_n[2], S.by_n[3], S.by_n[4], S.by_n[5], S.by_n[6], S.past,
         g_checks, g_failures);
  return g_failures ? 1 : 0;
}
