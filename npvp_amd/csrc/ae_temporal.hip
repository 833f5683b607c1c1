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
//   Entry points: npvp_temporal_attn_fwd / _bwd, 1 <= T <= 32 (TA_MAX_T), what is described above; npvp_temporal_attn_long_fwd /
// _bwd, any T >= 1: the same launches up to 32 frames, above that the key-tiled kernels in the second half of this file (one forward
// launch; a dq launch that also fills the caller's scratch D [2][rows], then a dk / dv launch), whose LDS does not depend on T.
#include "common.h"
#include "ae_attn_dims.h"

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

// ---- clips of more than TA_MAX_T frames: the same problem with the keys tiled (npvp_temporal_attn_long_*) ---------------------------
// A workgroup owns PT pixels x one tile of TT frames and walks the other side of the T x T score block in tiles of TT frames.  Both
// are chosen on the host: TT is the clip cut into the fewest equal tiles of at most MAX_TT = 32 frames (16 at (64, 256)) - 17 at
// T = 33, 20 at 40, 25 at 50, the last tile is shorter than the others by less than the number of tiles - and PT fills the LDS budget at that TT;
// the LDS of a workgroup is bounded by the MAX_TT figure whatever T is.  Frames past T in the last tile and pixels past HW are left
// out by the loop bounds: nothing is loaded, computed or stored for them (a key past T has P = 0, a query past T contributes nothing).
//   forward (per pixel tile x query tile): sweep 1 over the key tiles for the row's running max m and sum l (l rescaled by
// exp(m_old - m_new) when the max rises; tile 0 holds key 0, so m is finite from the first tile on), lse = m + log l; sweep 2, per
// <= 128 column chunk of v, accumulates exp(s - m) / l * v over the key tiles.
//   backward, D [2][rows] = row sums of P | D:  dq pass (per pixel tile x query tile): sweep 1 over the key tiles for sum_j P and
// sum_j P dP (P = exp(s - lse), dP = go v^T), written to D as sum P and D = sum P dP / sum P; sweep 2 for dS = Phat (dP - D) and
// dq += dS k.  dk / dv pass (per pixel tile x key tile) over the query tiles with lse, sum P and D read back: dv += Phat^T go per
// column chunk, then dk += dS^T q.  Accumulators live in LDS, each element owned by one thread from the first tile to the last, which
// stores it: every output element is written exactly once, sums run in tile order (bit-identical on repeated runs), no atomics.
constexpr int TL_LDS_LIMIT = 64 * 1024;

template <int A, int V>
struct TL {
  using C = TA<A, V>;
  static constexpr int MAX_TT = A == 64 ? 16 : 32;     // most frames of a query / key tile
  // frames of a tile: the fewest tiles of at most MAX_TT frames, of equal size (the last one may be shorter)
  static int frames(int T) {
    const int nt = (T + MAX_TT - 1) / MAX_TT;
    return (T + nt - 1) / nt;
  }
  // floats of LDS per pixel at TT frames per tile (scores in rows of TT + 1).  forward: q, k, v chunk, o chunk, scores, m, 1/l;
  // backward (both passes): q, k, v chunk (dv accumulator in the dk / dv pass's first phase), go chunk, P, dP, dq / dk accumulator,
  // lse, 1 / sum P, D.  (The accumulator behind the two score tiles stays 16-byte aligned: TT (TT + 1) is even.)
  static constexpr int pixel_floats(int TT, bool bwd) {
    return bwd ? TT * (3 * C::AP + 2 * C::VP + 2 * (TT + 1) + 3) : TT * (2 * C::AP + 2 * C::VP + (TT + 1) + 2);
  }
  static_assert(4 * pixel_floats(MAX_TT, false) <= TL_LDS_LIMIT && 4 * pixel_floats(MAX_TT, true) <= TL_LDS_LIMIT,
                "one pixel's tile must fit 64 KB of LDS");
  static int tile(int TT, int HW, bool bwd) {
    int pt = TA_LDS_BUDGET / (4 * pixel_floats(TT, bwd));
    pt = pt < 1 ? 1 : pt > TA_MAX_PT ? TA_MAX_PT : pt;
    return pt > HW ? HW : pt;
  }
};

struct TLGeo {
  int T, HW, PT, TT, ptiles, ttiles;   // pixel tiles of a clip, frame tiles of a clip
  long long frame0;                    // first row of this workgroup's clip at t = 0, plus the tile's first pixel
  int live, t0, tn;                    // pixels of this tile that exist; first frame and frames of this workgroup's own frame tile
  __device__ __forceinline__ void locate() {
    const int b = blockIdx.x / ttiles, ft = blockIdx.x - b * ttiles;
    const int n = b / ptiles, p0 = (b - n * ptiles) * PT;
    frame0 = (long long)n * T * HW + p0;
    live = HW - p0 < PT ? HW - p0 : PT;
    t0 = ft * TT;
    tn = T - t0 < TT ? T - t0 : TT;
  }
  __device__ __forceinline__ long long row(int t, int p) const { return frame0 + (long long)t * HW + p; }
};

// COLS columns (from column c0) of frames t0 .. t0 + tn of the live pixels -> dst[(p TT + t) * stride + c]
template <int COLS>
__device__ __forceinline__ void tl_load(const TLGeo& g, const float* __restrict__ src, long long ld, int c0, int t0, int tn, float* dst,
                                        int stride) {
  constexpr int C4 = COLS / 4;
  const int count = tn * g.live * C4;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c4 = e % C4, r = e / C4, p = r % g.live, t = r / g.live;
    st4(dst + (p * g.TT + t) * stride + 4 * c4, ld4(src + g.row(t0 + t, p) * ld + c0 + 4 * c4));
  }
}

// f(p TT + i, j, a[p][i][:] . b[p][j][:] over COLS columns) for i < qn, j < kn of the live pixels, one thread per (p, i, j): the same
// thread for the same (p, i, j) in every call with the same qn, kn
template <int COLS, class F>
__device__ __forceinline__ void tl_dots(const TLGeo& g, const float* a, const float* b, int stride, int qn, int kn, F f) {
  const int count = g.live * qn * kn;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int j = e % kn, r = e / kn, i = r % qn, p = r / qn;
    const float* ar = a + (p * g.TT + i) * stride;
    const float* br = b + (p * g.TT + j) * stride;
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < COLS; c += 4) {
      const float4 x = ld4(ar + c), y = ld4(br + c);
      s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    f(p * g.TT + i, j, s);
  }
}

// acc[p][t][:] (+)= sum_{u < un} w(p, t, u) * src[p][u][:] for the tn frames of the workgroup's own tile, w = W[(p TT + t) SP + u]
// (TRANS: W[(p TT + u) SP + t]); first: start from 0; last: the sum goes to dst row(t0 + t, p), columns c0 .. c0 + COLS, not to acc.
// One thread owns an element of acc through every call.
template <int COLS, bool TRANS>
__device__ __forceinline__ void tl_mix(const TLGeo& g, const float* W, const float* src, int stride, int un, float* acc, bool first,
                                       bool last, float* __restrict__ dst, long long ld, int c0) {
  constexpr int C4 = COLS / 4;
  const int SP = g.TT + 1, count = g.tn * g.live * C4;
  for (int e = threadIdx.x; e < count; e += 256) {
    const int c4 = e % C4, r = e / C4, p = r % g.live, t = r / g.live;
    const float* w = TRANS ? W + p * g.TT * SP + t : W + (p * g.TT + t) * SP;
    const float* s = src + p * g.TT * stride + 4 * c4;
    float* own = acc + (p * g.TT + t) * stride + 4 * c4;
    float4 sum = first ? make_float4(0.f, 0.f, 0.f, 0.f) : ld4(own);
    for (int u = 0; u < un; ++u) {
      const float wu = TRANS ? w[u * SP] : w[u];
      const float4 x = ld4(s + u * stride);
      sum.x = fmaf(wu, x.x, sum.x); sum.y = fmaf(wu, x.y, sum.y); sum.z = fmaf(wu, x.z, sum.z); sum.w = fmaf(wu, x.w, sum.w);
    }
    if (last) st4(dst + g.row(g.t0 + t, p) * ld + c0 + 4 * c4, sum);
    else st4(own, sum);
  }
}

template <int A, int V>
__global__ void __launch_bounds__(256) temporal_attn_long_fwd_kernel(const float* __restrict__ q, long long ldq,
                                                                     const float* __restrict__ k, long long ldk,
                                                                     const float* __restrict__ v, long long ldv, float* __restrict__ o,
                                                                     long long ldo, float* __restrict__ lse, TLGeo g) {
  using C = TA<A, V>;
  extern __shared__ float4 ta_lds4[];
  g.locate();
  const int T = g.T, TT = g.TT, SP = TT + 1, R = g.PT * TT, qn = g.tn, rows = g.live * qn;
  float* Qs = reinterpret_cast<float*>(ta_lds4);
  float* Ks = Qs + R * C::AP;
  float* Vs = Ks + R * C::AP;
  float* Os = Vs + R * C::VP;
  float* Ss = Os + R * C::VP;
  float* Ms = Ss + R * SP;
  float* Ls = Ms + R;
  tl_load<A>(g, q, ldq, 0, g.t0, qn, Qs, C::AP);
  for (int k0 = 0; k0 < T; k0 += TT) {                               // sweep 1: running max and sum of every row
    const int kn = T - k0 < TT ? T - k0 : TT;
    __syncthreads();
    tl_load<A>(g, k, ldk, 0, k0, kn, Ks, C::AP);
    __syncthreads();
    tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ss[r * SP + j] = s; });
    __syncthreads();
    for (int e = threadIdx.x; e < rows; e += 256) {                  // one row (p, i) per thread, the same thread in every tile
      const int p = e / qn, r = p * TT + e - p * qn;
      const float* s = Ss + r * SP;
      float mx = s[0];
      for (int j = 1; j < kn; ++j) mx = fmaxf(mx, s[j]);
      float l = 0.f;
      if (k0) {
        const float old = Ms[r];
        mx = fmaxf(mx, old);
        l = Ls[r] * expf(old - mx);
      }
      for (int j = 0; j < kn; ++j) l += expf(s[j] - mx);
      Ms[r] = mx;
      Ls[r] = l;
    }
  }
  for (int e = threadIdx.x; e < rows; e += 256) {
    const int p = e / qn, i = e - p * qn, r = p * TT + i;
    const float l = Ls[r];
    lse[g.row(g.t0 + i, p)] = Ms[r] + logf(l);
    Ls[r] = 1.f / l;
  }
  for (int c0 = 0; c0 < V; c0 += C::VC) {                            // sweep 2: o = sum over the key tiles of exp(s - m) / l * v
    for (int k0 = 0; k0 < T; k0 += TT) {
      const int kn = T - k0 < TT ? T - k0 : TT;
      __syncthreads();
      tl_load<A>(g, k, ldk, 0, k0, kn, Ks, C::AP);
      tl_load<C::VC>(g, v, ldv, c0, k0, kn, Vs, C::VP);
      __syncthreads();
      tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ss[r * SP + j] = expf(s - Ms[r]) * Ls[r]; });
      __syncthreads();
      tl_mix<C::VC, false>(g, Ss, Vs, C::VP, kn, Os, k0 == 0, k0 + TT >= T, o, ldo, c0);
    }
  }
}

// dP tile = go[p][i][:] . v[p][j][:] over the V columns in chunks of VC (v: key frames k0 .., go: query frames q0 ..), then
// done(r, j, dP) per element; Gs keeps the one chunk of a V <= 128 shape when `have_go` says it is already there
template <int A, int V, class F>
__device__ __forceinline__ void tl_dp(const TLGeo& g, const float* __restrict__ v, long long ldv, const float* __restrict__ go,
                                      long long ldgo, int q0, int qn, int k0, int kn, bool have_v, bool have_go, float* Vs, float* Gs,
                                      float* dPs, F done) {
  using C = TA<A, V>;
  const int SP = g.TT + 1;
  for (int c0 = 0; c0 < V; c0 += C::VC) {
    __syncthreads();
    if (!have_v) tl_load<C::VC>(g, v, ldv, c0, k0, kn, Vs, C::VP);
    if (!have_go) tl_load<C::VC>(g, go, ldgo, c0, q0, qn, Gs, C::VP);
    __syncthreads();
    if (c0 + C::VC >= V) tl_dots<C::VC>(g, Gs, Vs, C::VP, qn, kn, [&](int r, int j, float s) { done(r, j, c0 ? dPs[r * SP + j] + s : s); });
    else tl_dots<C::VC>(g, Gs, Vs, C::VP, qn, kn, [&](int r, int j, float s) { dPs[r * SP + j] = c0 ? dPs[r * SP + j] + s : s; });
  }
}

template <int A, int V>
__global__ void __launch_bounds__(256) temporal_attn_long_dq_kernel(const float* __restrict__ q, long long ldq,
                                                                    const float* __restrict__ k, long long ldk,
                                                                    const float* __restrict__ v, long long ldv,
                                                                    const float* __restrict__ go, long long ldgo,
                                                                    const float* __restrict__ lse, float* __restrict__ D,
                                                                    long long total, float* __restrict__ dq, long long lddq, TLGeo g) {
  using C = TA<A, V>;
  constexpr bool ONE = V == C::VC;                                   // one chunk: the tile's go rows are loaded once
  extern __shared__ float4 ta_lds4[];
  g.locate();
  const int T = g.T, TT = g.TT, SP = TT + 1, R = g.PT * TT, qn = g.tn, rows = g.live * qn;
  float* Qs = reinterpret_cast<float*>(ta_lds4);
  float* Ks = Qs + R * C::AP;
  float* Vs = Ks + R * C::AP;
  float* Gs = Vs + R * C::VP;
  float* Ps = Gs + R * C::VP;
  float* dPs = Ps + R * SP;
  float* Acc = dPs + R * SP;
  float* Lr = Acc + R * C::AP;
  float* Sr = Lr + R;
  float* Dr = Sr + R;
  tl_load<A>(g, q, ldq, 0, g.t0, qn, Qs, C::AP);
  for (int e = threadIdx.x; e < rows; e += 256) {
    const int p = e / qn, i = e - p * qn;
    Lr[p * TT + i] = lse[g.row(g.t0 + i, p)];
  }
  for (int k0 = 0; k0 < T; k0 += TT) {                               // sweep 1: sum_j P and sum_j P dP of every row
    const int kn = T - k0 < TT ? T - k0 : TT;
    __syncthreads();
    tl_load<A>(g, k, ldk, 0, k0, kn, Ks, C::AP);
    __syncthreads();
    tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ps[r * SP + j] = expf(s - Lr[r]); });
    tl_dp<A, V>(g, v, ldv, go, ldgo, g.t0, qn, k0, kn, false, ONE && k0 > 0, Vs, Gs, dPs,
                [&](int r, int j, float d) { dPs[r * SP + j] = d; });
    __syncthreads();
    for (int e = threadIdx.x; e < rows; e += 256) {
      const int p = e / qn, r = p * TT + e - p * qn;
      float l = k0 ? Sr[r] : 0.f, d = k0 ? Dr[r] : 0.f;
      for (int j = 0; j < kn; ++j) { l += Ps[r * SP + j]; d = fmaf(Ps[r * SP + j], dPs[r * SP + j], d); }
      Sr[r] = l;
      Dr[r] = d;
    }
  }
  for (int e = threadIdx.x; e < rows; e += 256) {
    const int p = e / qn, i = e - p * qn, r = p * TT + i;
    const float l = Sr[r], inv = 1.f / l, d = Dr[r] * inv;
    const long long gr = g.row(g.t0 + i, p);
    D[gr] = l;
    D[total + gr] = d;
    Sr[r] = inv;
    Dr[r] = d;
  }
  for (int k0 = 0; k0 < T; k0 += TT) {                               // sweep 2: dS = Phat (dP - D), dq += dS k
    const int kn = T - k0 < TT ? T - k0 : TT;
    __syncthreads();
    tl_load<A>(g, k, ldk, 0, k0, kn, Ks, C::AP);
    __syncthreads();
    tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ps[r * SP + j] = expf(s - Lr[r]) * Sr[r]; });
    tl_dp<A, V>(g, v, ldv, go, ldgo, g.t0, qn, k0, kn, false, ONE, Vs, Gs, dPs,
                [&](int r, int j, float d) { dPs[r * SP + j] = Ps[r * SP + j] * (d - Dr[r]); });
    __syncthreads();
    tl_mix<A, false>(g, dPs, Ks, C::AP, kn, Acc, k0 == 0, k0 + TT >= T, dq, lddq, 0);
  }
}

template <int A, int V>
__global__ void __launch_bounds__(256) temporal_attn_long_dkv_kernel(const float* __restrict__ q, long long ldq,
                                                                     const float* __restrict__ k, long long ldk,
                                                                     const float* __restrict__ v, long long ldv,
                                                                     const float* __restrict__ go, long long ldgo,
                                                                     const float* __restrict__ lse, const float* __restrict__ D,
                                                                     long long total, float* __restrict__ dk, long long lddk,
                                                                     float* __restrict__ dv, long long lddv, TLGeo g) {
  using C = TA<A, V>;
  constexpr bool ONE = V == C::VC;                                   // one chunk: the tile's v rows are loaded once
  extern __shared__ float4 ta_lds4[];
  g.locate();
  const int T = g.T, TT = g.TT, SP = TT + 1, R = g.PT * TT, kn = g.tn;
  float* Qs = reinterpret_cast<float*>(ta_lds4);
  float* Ks = Qs + R * C::AP;
  float* Vs = Ks + R * C::AP;                                        // the dv accumulator of the first phase
  float* Gs = Vs + R * C::VP;
  float* Ps = Gs + R * C::VP;
  float* dPs = Ps + R * SP;
  float* Acc = dPs + R * SP;
  float* Lr = Acc + R * C::AP;
  float* Sr = Lr + R;
  float* Dr = Sr + R;
  tl_load<A>(g, k, ldk, 0, g.t0, kn, Ks, C::AP);
  auto stats = [&](int q0, int qn) {                                 // lse, 1 / sum P and D of the query tile's rows
    for (int e = threadIdx.x; e < g.live * qn; e += 256) {
      const int p = e / qn, i = e - p * qn, r = p * TT + i;
      const long long gr = g.row(q0 + i, p);
      Lr[r] = lse[gr];
      Sr[r] = 1.f / D[gr];
      Dr[r] = D[total + gr];
    }
  };
  for (int c0 = 0; c0 < V; c0 += C::VC) {                            // dv = sum over the query tiles of Phat^T go, per column chunk
    for (int q0 = 0; q0 < T; q0 += TT) {
      const int qn = T - q0 < TT ? T - q0 : TT;
      __syncthreads();
      tl_load<A>(g, q, ldq, 0, q0, qn, Qs, C::AP);
      tl_load<C::VC>(g, go, ldgo, c0, q0, qn, Gs, C::VP);
      stats(q0, qn);
      __syncthreads();
      tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ps[r * SP + j] = expf(s - Lr[r]) * Sr[r]; });
      __syncthreads();
      tl_mix<C::VC, true>(g, Ps, Gs, C::VP, qn, Vs, q0 == 0, q0 + TT >= T, dv, lddv, c0);
    }
  }
  for (int q0 = 0; q0 < T; q0 += TT) {                               // dk = sum over the query tiles of dS^T q
    const int qn = T - q0 < TT ? T - q0 : TT;
    __syncthreads();
    tl_load<A>(g, q, ldq, 0, q0, qn, Qs, C::AP);
    stats(q0, qn);
    __syncthreads();
    tl_dots<A>(g, Qs, Ks, C::AP, qn, kn, [&](int r, int j, float s) { Ps[r * SP + j] = expf(s - Lr[r]) * Sr[r]; });
    tl_dp<A, V>(g, v, ldv, go, ldgo, q0, qn, g.t0, kn, ONE && q0 > 0, false, Vs, Gs, dPs,
                [&](int r, int j, float d) { dPs[r * SP + j] = Ps[r * SP + j] * (d - Dr[r]); });
    __syncthreads();
    tl_mix<A, true>(g, dPs, Qs, C::AP, qn, Acc, q0 == 0, q0 + TT >= T, dk, lddk, 0);
  }
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

// tiled: the npvp_temporal_attn_long_* entry points, whose T has no bound of its own
static int ta_check_shape(const char* name, int N, int T, int HW, int A, int V, bool tiled = false) {
  if (tiled) TA_REQUIRE(T >= 1, "%s: T = %d, a clip has T >= 1 frames", name, T);
  else TA_REQUIRE(T >= 1 && T <= TA_MAX_T, "%s: T = %d, 1 <= T <= %d frames per clip (longer clips need key tiling)", name, T, TA_MAX_T);
  TA_REQUIRE(N >= 1 && HW >= 1, "%s: N = %d, HW = %d must be >= 1", name, N, HW);
  TA_REQUIRE(npvp_ae_attn_dims(A, V), "%s: (attn dim, value dim) = (%d, %d) must be (8,32), (16,64), (32,128) or (64,256)", name, A, V);
  TA_REQUIRE((long long)N * T * HW < (1ll << 31), "%s: too many rows, N*T*HW = %lld (< 2^31)", name, (long long)N * T * HW);
  return NPVP_OK;
}

static int ta_check_operand(const char* name, const char* what, const void* p, long long ld, int cols) {
  TA_REQUIRE(p != nullptr, "%s: null buffer %s", name, what);
  TA_REQUIRE(ta_aligned(p), "%s: %s = %p is not 16-byte aligned", name, what, p);
  TA_REQUIRE(ld >= cols && ld % 4 == 0, "%s: leading dimension of %s = %lld must be >= %d and a multiple of 4", name, what, ld, cols);
  return NPVP_OK;
}

// MACRO(A, V) for the pair of ae_attn_dims.h that ta_check_shape has let through
#define TA_CASE(a, vv, MACRO) if (A == a) MACRO(a, vv) else
#define TA_DISPATCH(MACRO) NPVP_AE_ATTN_DIMS(TA_CASE, MACRO) {}

static TAGeo ta_geo(int T, int HW, int PT) {
  TAGeo g;
  g.T = T; g.HW = HW; g.PT = PT; g.tiles = (HW + PT - 1) / PT; g.frame0 = 0; g.live = 0;
  return g;
}

// the one-tile kernels (1 <= T <= TA_MAX_T), arguments already checked
static int ta_launch_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                         long long ldo, float* lse, int N, int T, int HW, int A, int V, hipStream_t stream) {
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

static int ta_launch_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, const float* go,
                         long long ldgo, const float* lse, float* dq, long long lddq, float* dk, long long lddk, float* dv,
                         long long lddv, int N, int T, int HW, int A, int V, hipStream_t stream) {
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

// what the forward and the backward check first, in this order: the shape, then the operands q, k, v
static int ta_check_qkv(const char* name, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                        int N, int T, int HW, int A, int V, bool tiled) {
  if (int rc = ta_check_shape(name, N, T, HW, A, V, tiled)) return rc;
  if (int rc = ta_check_operand(name, "q", q, ldq, A)) return rc;
  if (int rc = ta_check_operand(name, "k", k, ldk, A)) return rc;
  return ta_check_operand(name, "v", v, ldv, V);
}

static int ta_check_fwd(const char* name, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                        const float* o, long long ldo, const float* lse, int N, int T, int HW, int A, int V, bool tiled) {
  if (int rc = ta_check_qkv(name, q, ldq, k, ldk, v, ldv, N, T, HW, A, V, tiled)) return rc;
  if (int rc = ta_check_operand(name, "o", o, ldo, V)) return rc;
  TA_REQUIRE(lse != nullptr, "%s: null buffer lse", name);
  return NPVP_OK;
}

static int ta_check_bwd(const char* name, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                        const float* go, long long ldgo, const float* lse, const float* dq, long long lddq, const float* dk,
                        long long lddk, const float* dv, long long lddv, int N, int T, int HW, int A, int V, bool tiled) {
  if (int rc = ta_check_qkv(name, q, ldq, k, ldk, v, ldv, N, T, HW, A, V, tiled)) return rc;
  if (int rc = ta_check_operand(name, "go", go, ldgo, V)) return rc;
  if (int rc = ta_check_operand(name, "dq", dq, lddq, A)) return rc;
  if (int rc = ta_check_operand(name, "dk", dk, lddk, A)) return rc;
  if (int rc = ta_check_operand(name, "dv", dv, lddv, V)) return rc;
  TA_REQUIRE(lse != nullptr, "%s: null buffer lse", name);
  return NPVP_OK;
}

extern "C" int npvp_temporal_attn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                      float* o, long long ldo, float* lse, int N, int T, int HW, int A, int V, hipStream_t stream) {
  if (int rc = ta_check_fwd("npvp_temporal_attn_fwd", q, ldq, k, ldk, v, ldv, o, ldo, lse, N, T, HW, A, V, false)) return rc;
  return ta_launch_fwd(q, ldq, k, ldk, v, ldv, o, ldo, lse, N, T, HW, A, V, stream);
}

extern "C" int npvp_temporal_attn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                      const float* go, long long ldgo, const float* lse, float* dq, long long lddq, float* dk,
                                      long long lddk, float* dv, long long lddv, int N, int T, int HW, int A, int V, hipStream_t stream) {
  if (int rc = ta_check_bwd("npvp_temporal_attn_bwd", q, ldq, k, ldk, v, ldv, go, ldgo, lse, dq, lddq, dk, lddk, dv, lddv, N, T, HW, A, V,
                            false))
    return rc;
  return ta_launch_bwd(q, ldq, k, ldk, v, ldv, go, ldgo, lse, dq, lddq, dk, lddk, dv, lddv, N, T, HW, A, V, stream);
}

// ---- any T >= 1: the one-tile kernels up to TA_MAX_T (the same launches, the same bits, D untouched), the key-tiled kernels above
static TLGeo tl_geo(int T, int HW, int PT, int TT) {
  TLGeo g;
  g.T = T; g.HW = HW; g.PT = PT; g.TT = TT; g.ptiles = (HW + PT - 1) / PT; g.ttiles = (T + TT - 1) / TT;
  g.frame0 = 0; g.live = 0; g.t0 = 0; g.tn = 0;
  return g;
}

extern "C" int npvp_temporal_attn_long_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                           float* o, long long ldo, float* lse, int N, int T, int HW, int A, int V,
                                           hipStream_t stream) {
  if (int rc = ta_check_fwd("npvp_temporal_attn_long_fwd", q, ldq, k, ldk, v, ldv, o, ldo, lse, N, T, HW, A, V, true)) return rc;
  if (T <= TA_MAX_T) return ta_launch_fwd(q, ldq, k, ldk, v, ldv, o, ldo, lse, N, T, HW, A, V, stream);
#define TL_FWD(a, vv)                                                                                                              \
  {                                                                                                                                \
    const int TT = TL<a, vv>::frames(T);                                                                                           \
    const TLGeo g = tl_geo(T, HW, TL<a, vv>::tile(TT, HW, false), TT);                                                             \
    const size_t lds = sizeof(float) * (size_t)g.PT * TL<a, vv>::pixel_floats(TT, false);                                          \
    NPVP_LAUNCH((temporal_attn_long_fwd_kernel<a, vv>), dim3((unsigned)((long long)N * g.ptiles * g.ttiles)), dim3(256), lds,      \
                stream, q, ldq, k, ldk, v, ldv, o, ldo, lse, g);                                                                   \
  }
  TA_DISPATCH(TL_FWD)
#undef TL_FWD
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_temporal_attn_long_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                           const float* go, long long ldgo, const float* lse, float* D, float* dq, long long lddq,
                                           float* dk, long long lddk, float* dv, long long lddv, int N, int T, int HW, int A, int V,
                                           hipStream_t stream) {
  const char* name = "npvp_temporal_attn_long_bwd";
  if (int rc = ta_check_bwd(name, q, ldq, k, ldk, v, ldv, go, ldgo, lse, dq, lddq, dk, lddk, dv, lddv, N, T, HW, A, V, true)) return rc;
  TA_REQUIRE(D != nullptr, "%s: null buffer D", name);
  TA_REQUIRE(ta_aligned(D), "%s: D = %p is not 16-byte aligned", name, (const void*)D);
  if (T <= TA_MAX_T) return ta_launch_bwd(q, ldq, k, ldk, v, ldv, go, ldgo, lse, dq, lddq, dk, lddk, dv, lddv, N, T, HW, A, V, stream);
  const long long total = (long long)N * T * HW;
#define TL_BWD(a, vv)                                                                                                              \
  {                                                                                                                                \
    const int TT = TL<a, vv>::frames(T);                                                                                           \
    const TLGeo g = tl_geo(T, HW, TL<a, vv>::tile(TT, HW, true), TT);                                                              \
    const size_t lds = sizeof(float) * (size_t)g.PT * TL<a, vv>::pixel_floats(TT, true);                                           \
    const dim3 grid((unsigned)((long long)N * g.ptiles * g.ttiles));                                                               \
    NPVP_LAUNCH((temporal_attn_long_dq_kernel<a, vv>), grid, dim3(256), lds, stream, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D,     \
                total, dq, lddq, g);                                                                                               \
    NPVP_LAUNCH((temporal_attn_long_dkv_kernel<a, vv>), grid, dim3(256), lds, stream, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D,    \
                total, dk, lddk, dv, lddv, g);                                                                                     \
  }
  TA_DISPATCH(TL_BWD)
#undef TL_BWD
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
