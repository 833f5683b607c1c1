// Parameter-gradient partials, host side.  A backward kernel with a parameter gradient leaves partial rows [nb][ncols] in its
// workspace; a SumRowsJob says where they start and which gradient slices their column sums go to.  Each family has ONE layout
// function (ln_partials / fln_partials in norm.hip, mid_partials / dw_partials in mlpdw.hip, colsum_partials in elementwise.hip)
// that its producer, its *_workspace_bytes query, its *_reduce and its *_reduce_job all read.
#pragma once
#include <string.h>
#include "common.h"

int npvp_reduce_mid_launch(const float* in, float* out, int A, int B, long long Cc, float scale, hipStream_t stream, int accumulate = 0);   // elementwise.hip

namespace npvp {

struct SumRowsJob {
  const float* in; float* out; float* out_b;   // out_b (nullable): columns >= split go to out_b[c - split]
  int nb, stride, ncols, split;
  int accum;                                   // 1: += into out / out_b
  int mode;                                    // 0 plain; 1: depthwise-conv partials [10][Ch] (ncols = 10 Ch, split = Ch): tap t < 9 of channel c
                                               //    -> out[c*9 + t], the bias row -> out_b[c]   (mid_bwd_reduce_into_kernel's map)
};
static_assert(sizeof(SumRowsJob) == 48, "a job is 48 bytes (npvp_amd/ops.py ReduceQueue packs them back to back)");
constexpr int SRJ_MAX = 40;                    // jobs per launch of npvp_sum_rows_multi

// (items, chunks wanted) -> items per chunk and the chunks that are not empty then (160 frames in 16: 10 x 16; 70 in 16: 5 x 14)
struct ChunkSplit { int per, n; };
inline ChunkSplit split_chunks(long long items, int wanted) {
  if (wanted < 1) return {0, 0};
  const int fpc = (int)((items + wanted - 1) / wanted);
  return {fpc, (int)((items + fpc - 1) / fpc)};
}

// The partials of one producer call: rows [chunks][ncols], `lead` floats into the workspace.  job.in = their start, job.nb = the
// chunks used, per = the items a chunk walks, bytes = what the workspace query reports (the chunks WANTED: never less than used).
struct Partials { SumRowsJob job; int per; long long bytes; float* part() const { return const_cast<float*>(job.in); } };
inline Partials make_partials(const void* ws, long long lead, long long items, int wanted, int ncols, float* out, int accumulate,
                              float* out_b = nullptr, int split = 0, int mode = 0) {
  const ChunkSplit cs = split_chunks(items, wanted);
  return {{ws ? (const float*)ws + lead : nullptr, out, out_b, cs.n, ncols, ncols, split, accumulate ? 1 : 0, mode}, cs.per,
          (lead + (long long)wanted * ncols) * 4};
}
inline int put_job(void* job, const SumRowsJob& j) { memcpy(job, &j, sizeof(j)); return NPVP_OK; }   // what a *_reduce_job returns

// out[c] (+)= sum_b in[b*stride + c]; columns >= split go to out_b[c - split] (two parameter gradients from one partial buffer
// in one launch).  Mode-0 jobs only.  Defined in norm.hip, next to the plan that picks the kernel (plan_sum_rows).
int launch_sum_rows(const SumRowsJob& j, hipStream_t stream);

// The tail of every entry point that reduces: accumulate == 2 leaves the partials to the caller, anything else sums them now
// (a *_reduce entry point passes 0: it always sums; whether it adds is job.accum).
inline int finish_partials(const SumRowsJob& j, int accumulate, hipStream_t stream, const char* error) {
  if (accumulate == 2 || launch_sum_rows(j, stream) == NPVP_OK) return NPVP_OK;
  npvp_set_error(error);
  return NPVP_ERR_LAUNCH;
}

}  // namespace npvp
