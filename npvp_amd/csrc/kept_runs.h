// The K-steps of a split-K weight gradient that a row skip keeps (GemmParams::rskip on gemm_wgrad_f16_body), dealt over the splits.
// Plain integer code, host and device: tools/kept_runs_check.cpp walks it against a brute-force list for every mask of up to 12 groups.
//
// The reduction dimension is `groups` row groups of `spg` K-steps each (a K-step = 16 rows); bit g of `keep` says group g is kept.
// The kept K-steps, in their real order, form one sequence of Kk = popcount(keep) * spg steps; split z of `splits` takes the z-th
// share of ceil(Kk / splits) of them (the last shares may be shorter or empty), and walks it as maximal RUNS of consecutive real
// K-steps - adjacent kept groups merge into one run.  A function of (keep, spg, splits, z) alone.  With every group kept and
// groups * spg % splits == 0 the share of split z is the single run [z * Kk / splits, (z + 1) * Kk / splits): the chunk of a launch
// without a skip.
#pragma once

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace npvp {

struct KeptRuns {
  unsigned long long keep;   // bit g: group g is kept (g < 64)
  int spg;                   // K-steps per group
  int pos, end;              // this split's share [pos, end) of the kept sequence; pos advances run by run
};

__host__ __device__ inline KeptRuns kept_runs_of_split(unsigned long long keep, int spg, int splits, int z) {
  const int kk = __builtin_popcountll(keep) * spg;
  const int share = (kk + splits - 1) / splits;
  KeptRuns r;
  r.keep = keep; r.spg = spg;
  r.pos = z * share < kk ? z * share : kk;
  r.end = r.pos + share < kk ? r.pos + share : kk;
  return r;
}

// the next run of the share: real K-steps [k0, k0 + len), len >= 1; false when the share is used up
__host__ __device__ inline bool kept_runs_next(KeptRuns& r, int& k0, int& len) {
  if (r.pos >= r.end) return false;
  const int j = r.pos / r.spg, o = r.pos - j * r.spg;          // the j-th kept group, o steps into it
  unsigned long long m = r.keep;
  for (int i = 0; i < j; ++i) m &= m - 1;                      // (pos < popcount(keep) * spg: m keeps a set bit)
  const int g = __builtin_ctzll(m);
  const unsigned long long gap = ~(r.keep >> g);               // bit i: group g + i is NOT kept (the shift brings in zeros: "not kept")
  const int adj = gap ? __builtin_ctzll(gap) : 64;             // kept groups from g on without a gap (64: g == 0 and all 64 kept)
  const int avail = adj * r.spg - o;
  len = r.end - r.pos < avail ? r.end - r.pos : avail;
  k0 = g * r.spg + o;
  r.pos += len;
  return true;
}

}  // namespace npvp
