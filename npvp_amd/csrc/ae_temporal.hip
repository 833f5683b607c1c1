// Temporal non-local attention of the spatio-temporal autoencoder (learn_3d=True): the core of NonLocalAttenion1D.forward
// (ref/models/submodules.py:221-243) as Factorized3DConvAttn calls it on the (N*H*W, C, T) view of its frames (:62-66, :86-91):
// for every pixel, o = softmax(q k^T) v over that pixel's T frames, scores NOT scaled, one head.
//   The operands are read in place from the channels-last encoder's token rows: row(n, t, p) = (n T + t) HW + p, so the reference's
// two (N,T,C,H,W) <-> (N H W, C, T) permute copies per block are index arithmetic here.  A workgroup takes PT consecutive pixels of
// one clip: at a fixed t their rows are contiguous (PT * ld floats), the rows of the next frame lie HW * ld floats further on; the
// loads are float4 along the columns.  A pixel's q, k (T x A each) and a <= 128 column chunk of v (and of go in the backward) sit in
// LDS with its T x T score block; PT is chosen on the host from (A, V, T) so that a tile stays under 48 KB (one pixel at the widest
// shapes: 58 KB for the backward at T = 32, (64, 256)).  The last tile of a clip may be partial: its missing pixels load as zeros
// (nothing is read from them) and store nothing.
//   Arithmetic as csrc/ae_train.hip: fp32 VALU fmaf (the head widths are too narrow for an MFMA tile), max-subtracted softmax, lse
// saved.  The backward recomputes P = exp(s - lse), normalises the row (Phat = P / sum P, so the rounding of lse cannot scale a row)
// and takes D_i = sum_j Phat_ij dP_ij from the same Phat and dP.  A pixel's dq, dk and dv depend on that pixel's T rows only, so ONE
// kernel writes all three: no cross-workgroup reduction, no atomics, no workspace, no memset; every output element is written
// exactly once, in a fixed summation order (bit-identical on repeated runs).
#include "common.h"

#include <stdio.h>

namespace npvp {

constexpr int TA_MAX_T = 32;          // keys of a pixel are not tiled: T x T scores of a pixel stay in LDS
constexpr int TA_MAX_PT = 16;
constexpr int TA_LDS_BUDGET = 48 * 1024;

template <int A, int V>
struct TA {
  static constexpr int AP = A + 4;                     // LDS row strides: an odd number of 16-byte slots, conflict-free b128 reads
  static constexpr int VC = V < 128 ? V : 128;         // columns of v / go staged at a time
  static constexpr int VP = VC + 4;
  // floats of LDS per pixel: q, k, [v | v, go], [P | P, dP]
  static int pixel_floats(int T, bool bwd) { return T * (2 * AP + (bwd ? 2 : 1) * VP + (bwd ? 2 : 1) * (T + 1)); }
  static int tile(int T, int HW, bool bwd) {
    int pt = TA_LDS_BUDGET / (4 * pixel_floats(T, bwd));
    pt = pt < 1 ? 1 : pt > TA_MAX_PT ? TA_MAX_PT : pt;
    return pt > HW ? HW : pt;
  }
};

struct TAGeo {
  int T, HW, PT, tiles;                // tiles of a clip
  long long frame0;                    // first row of this workgroup's clip at t = 0, plus the tile's first pixel
  int live;                            // pixels of this tile that exist
  __device__ __forceinline__ void locate() {
    const int n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * PT;
    frame0 = (long long)n * T * HW + p0;
    live = HW - p0 < PT ? HW - p0 : PT;
  }
  __device__ __forceinline__ long long row(int t, int p) const { return frame0 + (long long)t * HW + p; }
};

// COLS columns (from column c0) of the tile's rows -> dst[(p T + t) * stride + c]; pixels past the clip's last load as zeros
template <int COLS>
__device__ __forceinline__ void ta_load(const TAGeo& g, const float* __restrict__ src, long long ld, int c0, float* dst, int stride) {
  constexpr int C4 = COLS / 4;
  const int count = g.T * g.PT * C4;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c4 = e % C4, r = e / C4, p = r % g.PT, t = r / g.PT;
    const float4 x = p < g.live ? ld4(src + g.row(t, p) * ld + c0 + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    st4(dst + (p * g.T + t) * stride + 4 * c4, x);
  }
}

// out[p][i][j] (+)= a[p][i][:] . b[p][j][:] over COLS columns, one thread per (p, i, j)
template <int COLS, bool ACCUM>
__device__ __forceinline__ void ta_dots(const TAGeo& g, const float* a, const float* b, int stride, float* out) {
  const int T = g.T, count = g.PT * T * T;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int j = e % T, r = e / T, i = r % T, p = r / T;
    const float* ar = a + (p * T + i) * stride;
    const float* br = b + (p * T + j) * stride;
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < COLS; c += 4) {
      const float4 x = ld4(ar + c), y = ld4(br + c);
      s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    float* d = out + (p * T + i) * (T + 1) + j;
    *d = ACCUM ? *d + s : s;
  }
}

// dst row(t, p), columns c0 .. c0 + COLS: sum_u w(p, t, u) * src[p][u][:]   with w = W[(p T + t)(T + 1) + u]  (TRANS: W[(p T + u)(T + 1) + t])
template <int COLS, bool TRANS>
__device__ __forceinline__ void ta_mix_store(const TAGeo& g, const float* W, const float* src, int stride, float* __restrict__ dst,
                                             long long ld, int c0) {
  constexpr int C4 = COLS / 4;
  const int T = g.T, count = T * g.PT * C4;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c4 = e % C4, r = e / C4, p = r % g.PT, t = r / g.PT;
    if (p >= g.live) continue;
    const float* w = TRANS ? W + p * T * (T + 1) + t : W + (p * T + t) * (T + 1);
    const float* s = src + p * T * stride + 4 * c4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u = 0; u < T; ++u) {
      const float wu = TRANS ? w[u * (T + 1)] : w[u];
      const float4 x = ld4(s + u * stride);
      acc.x = fmaf(wu, x.x, acc.x); acc.y = fmaf(wu, x.y, acc.y); acc.z = fmaf(wu, x.z, acc.z); acc.w = fmaf(wu, x.w, acc.w);
    }
    st4(dst + g.row(t, p) * ld + c0 + 4 * c4, acc);
  }
}

template <int A, int V>
__global__ void __launch_bounds__(256) temporal_attn_fwd_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ k,
                                                                long long ldk, const float* __restrict__ v, long long ldv,
                                                                float* __restrict__ o, long long ldo, float* __restrict__ lse, TAGeo g) {
  using C = TA<A, V>;
  extern __shared__ float4 ta_lds4[];
  g.locate();
  const int T = g.T, R = g.PT * T;
  float* Qs = reinterpret_cast<float*>(ta_lds4);
  float* Ks = Qs + R * C::AP;
  float* Vs = Ks + R * C::AP;
  float* Ps = Vs + R * C::VP;
  ta_load<A>(g, q, ldq, 0, Qs, C::AP);
  ta_load<A>(g, k, ldk, 0, Ks, C::AP);
  __syncthreads();
  ta_dots<A, false>(g, Qs, Ks, C::AP, Ps);
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += 256) {                      // one softmax row (p, i) per thread: T <= 32 scores
    float* s = Ps + r * (T + 1);
    float mx = s[0];
    for (int j = 1; j < T; ++j) mx = fmaxf(mx, s[j]);
    float l = 0.f;
    for (int j = 0; j < T; ++j) { const float e = expf(s[j] - mx); s[j] = e; l += e; }
    const float inv = 1.f / l;
    for (int j = 0; j < T; ++j) s[j] *= inv;
    const int p = r / T, i = r - p * T;
    if (p < g.live) lse[g.row(i, p)] = mx + logf(l);
  }
  for (int c0 = 0; c0 < V; c0 += C::VC) {
    __syncthreads();
    ta_load<C::VC>(g, v, ldv, c0, Vs, C::VP);
    __syncthreads();
    ta_mix_store<C::VC, false>(g, Ps, Vs, C::VP, o, ldo, c0);
  }
}

template <int A, int V>
__global__ void __launch_bounds__(256) temporal_attn_bwd_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ k,
                                                                long long ldk, const float* __restrict__ v, long long ldv,
                                                                const float* __restrict__ go, long long ldgo,
                                                                const float* __restrict__ lse, float* __restrict__ dq, long long lddq,
                                                                float* __restrict__ dk, long long lddk, float* __restrict__ dv,
                                                                long long lddv, TAGeo g) {
  using C = TA<A, V>;
  extern __shared__ float4 ta_lds4[];
  g.locate();
  const int T = g.T, R = g.PT * T;
  float* Qs = reinterpret_cast<float*>(ta_lds4);
  float* Ks = Qs + R * C::AP;
  float* Vs = Ks + R * C::AP;
  float* Gs = Vs + R * C::VP;
  float* Ps = Gs + R * C::VP;
  float* dPs = Ps + R * (T + 1);
  ta_load<A>(g, q, ldq, 0, Qs, C::AP);
  ta_load<A>(g, k, ldk, 0, Ks, C::AP);
  __syncthreads();
  ta_dots<A, false>(g, Qs, Ks, C::AP, Ps);                           // the forward's scores, bit for bit
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += 256) {                       // Phat = P / sum P, P = exp(s - lse)
    float* s = Ps + r * (T + 1);
    const int p = r / T, i = r - p * T;
    const float L = p < g.live ? lse[g.row(i, p)] : 0.f;
    float l = 0.f;
    for (int j = 0; j < T; ++j) { const float e = p < g.live ? expf(s[j] - L) : 0.f; s[j] = e; l += e; }
    const float inv = p < g.live ? 1.f / l : 0.f;
    for (int j = 0; j < T; ++j) s[j] *= inv;
  }
  for (int c0 = 0; c0 < V; c0 += C::VC) {                            // dP = go v^T summed over the chunks, dv = Phat^T go per chunk
    __syncthreads();
    ta_load<C::VC>(g, v, ldv, c0, Vs, C::VP);
    ta_load<C::VC>(g, go, ldgo, c0, Gs, C::VP);
    __syncthreads();
    if (c0 == 0) ta_dots<C::VC, false>(g, Gs, Vs, C::VP, dPs);
    else ta_dots<C::VC, true>(g, Gs, Vs, C::VP, dPs);
    ta_mix_store<C::VC, true>(g, Ps, Gs, C::VP, dv, lddv, c0);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < R; r += 256) {                       // dS = Phat (dP - D), D = sum_j Phat dP
    const float* s = Ps + r * (T + 1);
    float* d = dPs + r * (T + 1);
    float D = 0.f;
    for (int j = 0; j < T; ++j) D = fmaf(s[j], d[j], D);
    for (int j = 0; j < T; ++j) d[j] = s[j] * (d[j] - D);
  }
  __syncthreads();
  ta_mix_store<A, false>(g, dPs, Ks, C::AP, dq, lddq, 0);            // dq_i = sum_j dS_ij k_j
  ta_mix_store<A, true>(g, dPs, Qs, C::AP, dk, lddk, 0);             // dk_j = sum_i dS_ij q_i
}

}  // namespace npvp

using namespace npvp;

static bool ta_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// every refusal goes through NPVP_CHECK_ARG with the entry point's name and the offending value
#define TA_REQUIRE(cond, ...)                                  \
  do {                                                         \
    if (!(cond)) {                                             \
      char msg__[256];                                         \
      snprintf(msg__, sizeof(msg__), __VA_ARGS__);             \
      NPVP_CHECK_ARG(false, msg__);                            \
    }                                                          \
  } while (0)

static int ta_check_shape(const char* name, int N, int T, int HW, int A, int V) {
  TA_REQUIRE(T >= 1 && T <= TA_MAX_T, "%s: T = %d, 1 <= T <= %d frames per clip (longer clips need key tiling)", name, T, TA_MAX_T);
  TA_REQUIRE(N >= 1 && HW >= 1, "%s: N = %d, HW = %d must be >= 1", name, N, HW);
  TA_REQUIRE((A == 8 && V == 32) || (A == 16 && V == 64) || (A == 32 && V == 128) || (A == 64 && V == 256),
             "%s: (attn dim, value dim) = (%d, %d) must be (8,32), (16,64), (32,128) or (64,256)", name, A, V);
  TA_REQUIRE((long long)N * T * HW < (1ll << 31), "%s: too many rows, N*T*HW = %lld (< 2^31)", name, (long long)N * T * HW);
  return NPVP_OK;
}

static int ta_check_operand(const char* name, const char* what, const void* p, long long ld, int cols) {
  TA_REQUIRE(p != nullptr, "%s: null buffer %s", name, what);
  TA_REQUIRE(ta_aligned(p), "%s: %s = %p is not 16-byte aligned", name, what, p);
  TA_REQUIRE(ld >= cols && ld % 4 == 0, "%s: leading dimension of %s = %lld must be >= %d and a multiple of 4", name, what, ld, cols);
  return NPVP_OK;
}

#define TA_DISPATCH(MACRO) \
  if (A == 8) MACRO(8, 32) else if (A == 16) MACRO(16, 64) else if (A == 32) MACRO(32, 128) else MACRO(64, 256)

static TAGeo ta_geo(int T, int HW, int PT) {
  TAGeo g;
  g.T = T; g.HW = HW; g.PT = PT; g.tiles = (HW + PT - 1) / PT; g.frame0 = 0; g.live = 0;
  return g;
}

extern "C" int npvp_temporal_attn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                      float* o, long long ldo, float* lse, int N, int T, int HW, int A, int V, hipStream_t stream) {
  const char* name = "npvp_temporal_attn_fwd";
  if (int rc = ta_check_shape(name, N, T, HW, A, V)) return rc;
  if (int rc = ta_check_operand(name, "q", q, ldq, A)) return rc;
  if (int rc = ta_check_operand(name, "k", k, ldk, A)) return rc;
  if (int rc = ta_check_operand(name, "v", v, ldv, V)) return rc;
  if (int rc = ta_check_operand(name, "o", o, ldo, V)) return rc;
  TA_REQUIRE(lse != nullptr, "%s: null buffer lse", name);
#define TA_FWD(a, vv)                                                                                                              \
  {                                                                                                                                \
    const TAGeo g = ta_geo(T, HW, TA<a, vv>::tile(T, HW, false));                                                                  \
    const size_t lds = sizeof(float) * (size_t)g.PT * TA<a, vv>::pixel_floats(T, false);                                           \
    NPVP_LAUNCH((temporal_attn_fwd_kernel<a, vv>), dim3((unsigned)((long long)N * g.tiles)), dim3(256), lds, stream, q, ldq, k,    \
                ldk, v, ldv, o, ldo, lse, g);                                                                                      \
  }
  TA_DISPATCH(TA_FWD)
#undef TA_FWD
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_temporal_attn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                      const float* go, long long ldgo, const float* lse, float* dq, long long lddq, float* dk,
                                      long long lddk, float* dv, long long lddv, int N, int T, int HW, int A, int V, hipStream_t stream) {
  const char* name = "npvp_temporal_attn_bwd";
  if (int rc = ta_check_shape(name, N, T, HW, A, V)) return rc;
  if (int rc = ta_check_operand(name, "q", q, ldq, A)) return rc;
  if (int rc = ta_check_operand(name, "k", k, ldk, A)) return rc;
  if (int rc = ta_check_operand(name, "v", v, ldv, V)) return rc;
  if (int rc = ta_check_operand(name, "go", go, ldgo, V)) return rc;
  if (int rc = ta_check_operand(name, "dq", dq, lddq, A)) return rc;
  if (int rc = ta_check_operand(name, "dk", dk, lddk, A)) return rc;
  if (int rc = ta_check_operand(name, "dv", dv, lddv, V)) return rc;
  TA_REQUIRE(lse != nullptr, "%s: null buffer lse", name);
#define TA_BWD(a, vv)                                                                                                              \
  {                                                                                                                                \
    const TAGeo g = ta_geo(T, HW, TA<a, vv>::tile(T, HW, true));                                                                   \
    const size_t lds = sizeof(float) * (size_t)g.PT * TA<a, vv>::pixel_floats(T, true);                                            \
    NPVP_LAUNCH((temporal_attn_bwd_kernel<a, vv>), dim3((unsigned)((long long)N * g.tiles)), dim3(256), lds, stream, q, ldq, k,    \
                ldk, v, ldv, go, ldgo, lse, dq, lddq, dk, lddk, dv, lddv, g);                                                      \
  }
  TA_DISPATCH(TA_BWD)
#undef TA_BWD
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
