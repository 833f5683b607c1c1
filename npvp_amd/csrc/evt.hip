// The learned event token of the encoder (ref/models/VidHRFormer.py:35-42, ref/models/Predictor.py:343-344) on token rows [N][T][P][C]:
//   join : y[n, t < T] = x[n, t],  y[n, T] = token    (one [P, C] block for all clips, one per clip, or none: zeros)
//   split: y [N, T+1, P, C] -> x [N, T, P, C] and / or last [N, P, C]
// Each is the other's adjoint (the sum over clips of a shared token's gradient is npvp_reduce_mid on the split's `last`).  Both are
// HBM-bound copies built like gridpad.hip: 16-byte accesses, a capped grid with a grid-stride loop over rows, the row -> (clip, frame)
// decode once per row with a multiply-shift division (div_magic), two rows in flight per thread.  Every output element is written
// exactly once; no atomics but the amax words: bit-reproducible.
#include "common.h"

namespace npvp {

// The iteration space is `per_clip` rows for each of N clips; row i of it is row `base + i % per_clip` of its clip's T+1 frames.
struct EvtGeom {
  unsigned int per_clip, base;              // rows walked per clip, the first of them inside the clip's (T+1)*P rows
  unsigned int body, joined;                // T*P, (T+1)*P
  unsigned int P;
  unsigned int m_clip; int s_clip;          // magic of per_clip
};

struct EvtRow { unsigned int n, rem; };     // clip, row inside the clip's (T+1)*P rows

__device__ __forceinline__ EvtRow evt_decode(const EvtGeom& g, unsigned int i) {
  EvtRow r;
  r.n = div_by_magic(i, g.m_clip, g.s_clip);
  r.rem = i - r.n * g.per_clip + g.base;
  return r;
}

// source of joined row (n, rem): a row of x, a row of the token, or nullptr (zeros)
__device__ __forceinline__ const float* join_source(const EvtGeom& g, const EvtRow& r, const float* __restrict__ x, long long ld_x,
                                                    const float* __restrict__ token, long long ld_tok, long long tok_clip) {
  if (r.rem < g.body) return x ? x + ((long long)r.n * g.body + r.rem) * ld_x : nullptr;
  return token ? token + (long long)r.n * tok_clip + (long long)(r.rem - g.body) * ld_tok : nullptr;
}

// 256 threads = (256 >> lg) rows x (1 << lg) lanes of float4; lanes stride over the row when C/4 > lanes
__global__ __launch_bounds__(256) void evt_token_join_kernel(const float* __restrict__ x, long long ld_x, const float* __restrict__ token,
                                                             long long ld_tok, long long tok_clip, float* __restrict__ y, long long ld_y,
                                                             EvtGeom g, unsigned int rows, int c4n, int lg, float* __restrict__ amax) {
  __shared__ float ared[4];
  const unsigned int peek = amax_peek_block(amax);
  const int lanes = 1 << lg, lane = threadIdx.x & (lanes - 1);
  const unsigned int rpb = 256u >> lg, step = gridDim.x * rpb;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float am = 0.f;
  // (rows < 2^31 and step <= 2^19: r + step does not wrap; the iteration space IS the output: per_clip = joined, base = 0)
  for (unsigned int r = blockIdx.x * rpb + (threadIdx.x >> lg); r < rows; r += 2 * step) {
    const unsigned int r2 = r + step;
    const bool two = r2 < rows;
    const float* s1 = join_source(g, evt_decode(g, r), x, ld_x, token, ld_tok, tok_clip);
    const float* s2 = two ? join_source(g, evt_decode(g, r2), x, ld_x, token, ld_tok, tok_clip) : nullptr;
    for (int c = lane; c < c4n; c += lanes) {
      const float4 v1 = s1 ? ld4(s1 + 4 * c) : zero;
      const float4 v2 = s2 ? ld4(s2 + 4 * c) : zero;
      st4(y + (long long)r * ld_y + 4 * c, v1);
      if (two) st4(y + (long long)r2 * ld_y + 4 * c, v2);
      am = amax4(amax4(am, v1), v2);
    }
  }
  amax_slot_commit_block(amax, am, ared, peek);
}

// destination of joined row (n, rem): a row of x or a row of last; is_last tells which, and so which bound the row feeds
__device__ __forceinline__ float* split_dest(const EvtGeom& g, const EvtRow& r, float* __restrict__ x, long long ld_x,
                                             float* __restrict__ last, long long ld_last, bool& is_last) {
  is_last = r.rem >= g.body;
  if (!is_last) return x + ((long long)r.n * g.body + r.rem) * ld_x;
  return last + ((long long)r.n * g.P + (r.rem - g.body)) * ld_last;
}

__global__ __launch_bounds__(256) void evt_token_split_kernel(const float* __restrict__ y, long long ld_y, float* __restrict__ x,
                                                              long long ld_x, float* __restrict__ last, long long ld_last, EvtGeom g,
                                                              unsigned int rows, int c4n, int lg, float* __restrict__ x_amax,
                                                              float* __restrict__ last_amax) {
  __shared__ float ared_x[4], ared_l[4];
  const unsigned int peek_x = amax_peek_block(x_amax), peek_l = amax_peek_block(last_amax);
  const int lanes = 1 << lg, lane = threadIdx.x & (lanes - 1);
  const unsigned int rpb = 256u >> lg, step = gridDim.x * rpb;
  float am_x = 0.f, am_l = 0.f;
  for (unsigned int r = blockIdx.x * rpb + (threadIdx.x >> lg); r < rows; r += 2 * step) {
    const unsigned int r2 = r + step;
    const bool two = r2 < rows;
    const EvtRow e1 = evt_decode(g, r), e2 = evt_decode(g, two ? r2 : r);
    // (the host chose the iteration space so that every row walked belongs to a wanted output: d1, d2 are never null)
    bool l1, l2;
    float* d1 = split_dest(g, e1, x, ld_x, last, ld_last, l1);
    float* d2 = split_dest(g, e2, x, ld_x, last, ld_last, l2);
    const float* s1 = y + ((long long)e1.n * g.joined + e1.rem) * ld_y;
    const float* s2 = y + ((long long)e2.n * g.joined + e2.rem) * ld_y;
    for (int c = lane; c < c4n; c += lanes) {
      const float4 v1 = ld4(s1 + 4 * c);
      const float4 v2 = ld4(s2 + 4 * c);
      st4(d1 + 4 * c, v1);
      if (two) st4(d2 + 4 * c, v2);
      if (l1) am_l = amax4(am_l, v1); else am_x = amax4(am_x, v1);
      if (l2) am_l = amax4(am_l, v2); else am_x = amax4(am_x, v2);        // (without a second row v2 repeats v1: the bounds are unchanged)
    }
  }
  amax_slot_commit_block(x_amax, am_x, ared_x, peek_x);
  amax_slot_commit_block(last_amax, am_l, ared_l, peek_l);
}

// lanes per row: the smallest power of two >= C/4, at most 256
static inline int evt_lane_bits(int c4n) {
  int lg = 0;
  while (lg < 8 && (1 << lg) < c4n) ++lg;
  return lg;
}

static inline int evt_blocks(long long rows, int lg) {
  const long long rpb = 256 >> lg;
  long long b = (rows + rpb - 1) / rpb;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace npvp

using namespace npvp;

static const char* evt_check(int N, int T, int P, int C) {
  if (N <= 0 || T <= 0 || P <= 0 || C <= 0) return "evt token: bad shape";
  if (C % 4 != 0) return "evt token: C must be a multiple of 4";
  if ((long long)N * ((long long)T + 1) * P >= (1ll << 31)) return "evt token: row counts must fit 32 bits";
  return nullptr;
}

static inline bool evt_stride_ok(long long ld, int C) { return ld % 4 == 0 && ld >= C; }

static EvtGeom evt_geom(int T, int P, unsigned int per_clip, unsigned int base) {
  EvtGeom g;
  g.per_clip = per_clip; g.base = base;
  g.body = (unsigned int)T * (unsigned int)P; g.joined = g.body + (unsigned int)P; g.P = (unsigned int)P;
  div_magic(per_clip, g.m_clip, g.s_clip);
  return g;
}

extern "C" int npvp_evt_token_join(const float* x, long long ld_x, const float* token, long long ld_token, long long token_clip_stride,
                                   float* y, long long ld_y, int N, int T, int P, int C, float* y_amax, hipStream_t stream) {
  const char* why = evt_check(N, T, P, C);
  NPVP_CHECK_ARG(!why, why);
  NPVP_CHECK_ARG(evt_stride_ok(ld_y, C) && (!x || evt_stride_ok(ld_x, C)) && (!token || evt_stride_ok(ld_token, C)),
                 "evt token join: row strides must be multiples of 4 and at least C");
  NPVP_CHECK_ARG(!token || token_clip_stride == 0 || (token_clip_stride % 4 == 0 && token_clip_stride >= (long long)P * ld_token),
                 "evt token join: the token's clip stride must be 0 (one block for all clips) or a multiple of 4 that holds P rows");
  NPVP_CHECK_ARG(y, "evt token join: null buffer");
  NPVP_CHECK_ARG(((uintptr_t)x | (uintptr_t)token | (uintptr_t)y) % 16 == 0, "evt token join: buffers must be 16-byte aligned");
  const long long rows = (long long)N * (T + 1) * P;
  const int c4n = C / 4, lg = evt_lane_bits(c4n);
  const EvtGeom g = evt_geom(T, P, (unsigned int)((T + 1) * P), 0u);
  NPVP_LAUNCH(evt_token_join_kernel, dim3(evt_blocks(rows, lg)), dim3(256), 0, stream, x, ld_x, token, ld_token, token_clip_stride, y, ld_y,
              g, (unsigned int)rows, c4n, lg, y_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_evt_token_split(const float* y, long long ld_y, float* x, long long ld_x, float* last, long long ld_last, int N, int T,
                                    int P, int C, float* x_amax, float* last_amax, hipStream_t stream) {
  const char* why = evt_check(N, T, P, C);
  NPVP_CHECK_ARG(!why, why);
  NPVP_CHECK_ARG(evt_stride_ok(ld_y, C) && (!x || evt_stride_ok(ld_x, C)) && (!last || evt_stride_ok(ld_last, C)),
                 "evt token split: row strides must be multiples of 4 and at least C");
  NPVP_CHECK_ARG(y && (x || last), "evt token split: null buffer");
  NPVP_CHECK_ARG(((uintptr_t)y | (uintptr_t)x | (uintptr_t)last) % 16 == 0, "evt token split: buffers must be 16-byte aligned");
  // the rows walked per clip: all (T+1)*P when both outputs are wanted, the first T*P for x alone, the last P for `last` alone
  const unsigned int body = (unsigned int)T * (unsigned int)P;
  const unsigned int per_clip = (x && last) ? body + (unsigned int)P : (x ? body : (unsigned int)P);
  const long long rows = (long long)N * per_clip;
  const int c4n = C / 4, lg = evt_lane_bits(c4n);
  const EvtGeom g = evt_geom(T, P, per_clip, x ? 0u : body);
  NPVP_LAUNCH(evt_token_split_kernel, dim3(evt_blocks(rows, lg)), dim3(256), 0, stream, y, ld_y, x, ld_x, last, ld_last, g,
              (unsigned int)rows, c4n, lg, x ? x_amax : nullptr, last ? last_amax : nullptr);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
