// Exhaustive host check of csrc/kept_runs.h (the K-steps a row-skipping weight gradient keeps, dealt over its splits) against a
// brute-force list: every mask of 1 .. 12 groups, 1 .. 5 K-steps per group, 1 .. 17 splits - and a few 64-group masks.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kept_runs_check.cpp -o /tmp/kept_runs_check
//   /tmp/kept_runs_check          (prints the number of (mask, spg, splits) cases walked; exit status 1 and a line per mismatch)
#include <cstdio>
#include <vector>

#include "../npvp_amd/csrc/kept_runs.h"

using npvp::KeptRuns;

static long long g_cases = 0, g_bad = 0;

static void fail(const char* what, int groups, unsigned long long keep, int spg, int splits, int z) {
  if (++g_bad <= 20) std::printf("MISMATCH %s: groups %d keep %#llx spg %d splits %d z %d\n", what, groups, keep, spg, splits, z);
}

static void check(int groups, unsigned long long keep, int spg, int splits) {
  ++g_cases;
  std::vector<int> kept;                                   // the real K-steps of kept groups, in order
  for (int g = 0; g < groups; ++g)
    if ((keep >> g) & 1ull)
      for (int s = 0; s < spg; ++s) kept.push_back(g * spg + s);
  const int kk = (int)kept.size(), share = (kk + splits - 1) / splits;
  size_t at = 0;                                           // the shares, concatenated in z order, must be `kept`
  for (int z = 0; z < splits; ++z) {
    const int lo = z * share < kk ? z * share : kk, hi = lo + share < kk ? lo + share : kk;
    KeptRuns r = npvp::kept_runs_of_split(keep, spg, splits, z);
    int k0 = -1, len = -1, prev_end = -2, n = 0;
    while (npvp::kept_runs_next(r, k0, len)) {
      if (len < 1) { fail("empty run", groups, keep, spg, splits, z); return; }
      if (k0 <= prev_end) fail("runs not maximal or not ascending", groups, keep, spg, splits, z);     // (k0 == prev_end: should have merged)
      for (int i = 0; i < len; ++i, ++n) {
        if (at >= kept.size() || kept[at] != k0 + i) { fail("step", groups, keep, spg, splits, z); return; }
        ++at;
      }
      prev_end = k0 + len;
    }
    if (n != hi - lo) fail("share length", groups, keep, spg, splits, z);
    // nothing dropped and an even deal: today's chunk, one run
    if (kk == groups * spg && kk % splits == 0) {
      KeptRuns q = npvp::kept_runs_of_split(keep, spg, splits, z);
      int a, b;
      if (!(npvp::kept_runs_next(q, a, b) && a == z * (kk / splits) && b == kk / splits && !npvp::kept_runs_next(q, a, b)))
        fail("all kept is not the plain chunk", groups, keep, spg, splits, z);
    }
  }
  if (at != kept.size()) fail("steps left over", groups, keep, spg, splits, -1);
}

int main() {
  for (int groups = 1; groups <= 12; ++groups)
    for (unsigned long long keep = 0; keep < (1ull << groups); ++keep)
      for (int spg = 1; spg <= 5; ++spg)
        for (int splits = 1; splits <= 17; ++splits) check(groups, keep, spg, splits);
  // the 64-group edge: all kept (no zero bit to find), all but the ends, alternating, the top bit alone; and the "no skip" form
  // (one group of every K-step)
  const unsigned long long wide[] = {~0ull, ~0ull >> 1, ~0ull << 1, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull, 1ull << 63, 0ull,
                                     0xffffffff00000000ull, 0x00ffff0000ffff00ull};
  for (unsigned long long keep : wide)
    for (int spg : {1, 16, 48})
      for (int splits : {1, 8, 16, 64}) check(64, keep, spg, splits);
  for (int steps : {16, 64, 1024, 7168})
    for (int splits : {1, 8, 16, 64}) check(1, 1ull, steps, splits);
  std::printf("%lld cases, %lld mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
