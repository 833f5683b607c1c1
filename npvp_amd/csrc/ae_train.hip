// Training step of the Stage-1 autoencoder (ref/models/ResNetAutoEncoder.py:13-49 LitAE, its ResnetEncoder / ResnetDecoder and the
// NonLocalAttenion2D blocks of ref/models/submodules.py:98-176): everything on the step's hot path but the convolutions (MIOpen).
//   - training-mode BatchNorm2d fused with its ReLU and skip-add: statistics (fixed-order two-level sums in double, no atomics, no
//     memset) and apply are separate entry points, so that a data-parallel caller can all-reduce [sum x, sum x^2] in between;
//   - its backward: fixed-order sums of g' and g' * xhat, then one pass dx = w rstd (g' - sum g'/n - xhat sum g' xhat / n);
//   - the same two passes cut where synchronised BatchNorm exchanges (Lightning's sync_batchnorm=True,
//     ref/train_AutoEncoder_lightning.py:40-42): the forward from stat[2C+1] = [sum x, sum x^2, n] and the backward's dx from
//     sums[2C] = [sum g', sum g' xhat], both all-reduced by the caller, the element count n read on the device (uneven shards);
//   - the non-local attention core softmax(q k^T) v (unscaled scores) with the 2x2 max-pool of K / V fused into the loads, flash
//     style: online softmax forward, recomputation backward, the HW x HW/4 score matrix never leaves LDS; each pooled K / V gradient
//     goes to its window's arg-max (first maximum in row-major window order, as torch's max_pool2d); exact-tile kernels for the
//     four (C, grid) pairs of the shipped configs, and a masked general form of the same kernels for any other H x W grid (odd,
//     rectangular, not a power of two; floor pooling, the never-pooled last line / column gets dk = dv = 0 from a kernel);
//   - ReflectionPad2d forward and a gather-form backward (every input pixel sums its mirror images in a fixed order).
// Every kernel here is deterministic: no atomics, fixed summation order, bit-identical on repeated runs.
//   BatchNorm / pad layouts: 0 = channels-last [outer][C] (the encoder), 1 = NCHW planes [N*C][H*W] (the decoder).
// The attention runs on the f32 VALU (v_fma_f32): exact fp32 products at the same peak rate as the f32 MFMA (cdna_hip_programming §3),
// and the head dimensions here (8..64) are too narrow to fill an MFMA tile without padding.
#include "common.h"
#include "ae_attn_dims.h"

#include <stdlib.h>

namespace npvp {

constexpr int BN_MAX_PARTS = 1024;

// ----------------------------------------------------------------------------------------------------------------- BatchNorm

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// scale / shift of channel c: z = x * sc + sh, the SAME two fmaf in the forward and in the backward's ReLU-mask recomputation
__device__ __forceinline__ void bn_coef(const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ w,
                                        const float* __restrict__ b, int c, float& sc, float& sh) {
  sc = rstd[c] * w[c];
  sh = fmaf(-mean[c], sc, b[c]);
}

// the pair summed per channel.  MODE 0: (x, x^2).  MODE 1 (backward): (g', g' xhat), g' = g * act'(z) recomputed from x.
template <int MODE>
__device__ __forceinline__ void bn_pair(float x, float g, float mu, float rs, float sc, float sh, int act, double& s1, double& s2) {
  if (MODE == 0) {
    s1 += (double)x;
    s2 += (double)x * (double)x;
  } else {
    const float gp = (act == 1 && fmaf(x, sc, sh) <= 0.f) ? 0.f : g;
    s1 += (double)gp;
    s2 += (double)gp * (double)((x - mu) * rs);
  }
}

// layout 0: grid (ceil(C/64), P); lane = channel, the 4 waves stride over the part's rows.  part[p][2][C]
template <int MODE>
__global__ void __launch_bounds__(256) bn_part_rows_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ w, const float* __restrict__ b, int act,
                                                           long long R, int C, long long rows_per_part, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int p = blockIdx.y;
  const long long r0 = (long long)p * rows_per_part;
  const long long r1 = r0 + rows_per_part < R ? r0 + rows_per_part : R;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    float mu = 0.f, rs = 0.f, sc = 0.f, sh = 0.f;
    if (MODE == 1) { mu = mean[c]; rs = rstd[c]; bn_coef(mean, rstd, w, b, c, sc, sh); }
    for (long long r = r0 + wv; r < r1; r += 4) {
      const long long e = r * C + c;
      bn_pair<MODE>(x[e], MODE == 1 ? g[e] : 0.f, mu, rs, sc, sh, act, s1, s2);
    }
  }
  __shared__ double lds[2][4][64];
  lds[0][wv][lane] = s1;
  lds[1][wv][lane] = s2;
  __syncthreads();
  if (wv == 0 && c < C) {
    const double t1 = ((lds[0][0][lane] + lds[0][1][lane]) + lds[0][2][lane]) + lds[0][3][lane];
    const double t2 = ((lds[1][0][lane] + lds[1][1][lane]) + lds[1][2][lane]) + lds[1][3][lane];
    part[(long long)p * 2 * C + c] = t1;
    part[(long long)p * 2 * C + C + c] = t2;
  }
}

// layout 1: grid (C, P); the block sums planes n in its part of channel c (float4 over H*W, HW % 4 == 0)
template <int MODE>
__global__ void __launch_bounds__(256) bn_part_planes_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ w, const float* __restrict__ b, int act,
                                                             int N, int C, int HW, int planes_per_part, double* __restrict__ part) {
  const int c = blockIdx.x, p = blockIdx.y;
  const int n0 = p * planes_per_part;
  const int n1 = n0 + planes_per_part < N ? n0 + planes_per_part : N;
  float mu = 0.f, rs = 0.f, sc = 0.f, sh = 0.f;
  if (MODE == 1) { mu = mean[c]; rs = rstd[c]; bn_coef(mean, rstd, w, b, c, sc, sh); }
  double s1 = 0.0, s2 = 0.0;
  const int hw4 = HW >> 2;
  for (int n = n0; n < n1; ++n) {
    const long long base = ((long long)n * C + c) * HW;
    for (int i = threadIdx.x; i < hw4; i += 256) {
      const float4 v = ld4(x + base + 4 * i);
      float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == 1) gg = ld4(g + base + 4 * i);
      bn_pair<MODE>(v.x, gg.x, mu, rs, sc, sh, act, s1, s2);
      bn_pair<MODE>(v.y, gg.y, mu, rs, sc, sh, act, s1, s2);
      bn_pair<MODE>(v.z, gg.z, mu, rs, sc, sh, act, s1, s2);
      bn_pair<MODE>(v.w, gg.w, mu, rs, sc, sh, act, s1, s2);
    }
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  __shared__ double lds[2][4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { lds[0][wv] = s1; lds[1][wv] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(long long)p * 2 * C + c] = ((lds[0][0] + lds[0][1]) + lds[0][2]) + lds[0][3];
    part[(long long)p * 2 * C + C + c] = ((lds[1][0] + lds[1][1]) + lds[1][2]) + lds[1][3];
  }
}

// second level: sums[2][C] = sum over the P parts, one wave per channel and quantity (blockIdx.x): lane l sums parts l, l + 64, ...
// in order, then a fixed butterfly (a single thread per column walking 1024 parts took 59 us per call, measured)
__global__ void __launch_bounds__(64) bn_part_reduce_kernel(const double* __restrict__ part, int P, int C, double* __restrict__ sums) {
  const int i = blockIdx.x;
  double s = 0.0;
  for (int p = threadIdx.x; p < P; p += 64) s += part[(long long)p * 2 * C + i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) sums[i] = s;
}

// mean / rstd per channel: from the sums (training: batch statistics, running statistics updated as torch does - momentum,
// unbiased variance) or, with sums == null, from the running statistics (eval).  The element count per channel is `count`, or
// *count_dev when given (synchronised BatchNorm: the all-reduced total, known on the device only)
__global__ void bn_finalize_kernel(const double* __restrict__ sums, double count, const double* __restrict__ count_dev, float eps,
                                   float momentum, float* __restrict__ running_mean, float* __restrict__ running_var, int C,
                                   float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (count_dev) count = *count_dev;
  if (sums) {
    const double m = sums[c] / count;
    double var = sums[C + c] / count - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
      const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
  } else {
    mean[c] = running_mean[c];
    rstd[c] = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
  }
}

// backward: dw = sum g' xhat, db = sum g' (float) from the double sums
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ sums, int C, float* __restrict__ dw, float* __restrict__ db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  db[c] = (float)sums[c];
  dw[c] = (float)sums[C + c];
}

__device__ __forceinline__ float bn_out(float x, float sc, float sh, int act) {
  const float z = fmaf(x, sc, sh);
  return act == 1 ? fmaxf(z, 0.f) : z;
}

// dx of one element.  train: w rstd (g' - db/n - xhat dw/n); eval: w rstd g'
__device__ __forceinline__ float bn_dx(float x, float g, float mu, float rs, float sc, float sh, float k1, float k2, int act, int train) {
  const float gp = (act == 1 && fmaf(x, sc, sh) <= 0.f) ? 0.f : g;
  if (!train) return sc * gp;
  const float xh = (x - mu) * rs;
  return sc * (gp - k1 - xh * k2);
}

// elementwise passes (forward apply / backward dx).  layout 0: C4 = C/4 divides 256, each thread keeps its 4 channels' coefficients
// and strides over rows; layout 1: one block per plane (n, c), float4 over H*W.
// BWD 0: forward; 1: dx from this call's own dw / db (float) and the host's 1/n; 2: dx from all-reduced rsums[2][C] (double) and the
// device count *rcount, rounded to float exactly as BWD 1 rounds them (the same bits when the sums are this rank's own)
template <int BWD>
__device__ __forceinline__ void bn_k(const float* __restrict__ dw, const float* __restrict__ db, const double* __restrict__ rsums,
                                     float inv_n, int c, int C, float& k1, float& k2) {
  if (BWD == 2) { k1 = (float)rsums[c] * inv_n; k2 = (float)rsums[C + c] * inv_n; }
  else if (BWD == 1) { k1 = db[c] * inv_n; k2 = dw[c] * inv_n; }
  else { k1 = 0.f; k2 = 0.f; }
}

template <int BWD>
__global__ void __launch_bounds__(256) bn_elem_rows_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ res, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ w,
                                                           const float* __restrict__ b, const float* __restrict__ dw,
                                                           const float* __restrict__ db, const double* __restrict__ rsums,
                                                           const double* __restrict__ rcount, float inv_n, int act, int train,
                                                           long long R, int C, float* __restrict__ out) {
  if (BWD == 2) inv_n = (float)(1.0 / *rcount);
  const int C4 = C >> 2;
  const int rpb = 256 / C4;
  const int c = (threadIdx.x % C4) * 4;
  float sc[4], sh[4], mu[4], rs[4], k1[4], k2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    bn_coef(mean, rstd, w, b, c + u, sc[u], sh[u]);
    mu[u] = mean[c + u]; rs[u] = rstd[c + u];
    bn_k<BWD>(dw, db, rsums, inv_n, c + u, C, k1[u], k2[u]);
  }
  for (long long r = (long long)blockIdx.x * rpb + threadIdx.x / C4; r < R; r += (long long)gridDim.x * rpb) {
    const long long e = r * C + c;
    const float4 v = ld4(x + e);
    float o[4] = {v.x, v.y, v.z, v.w};
    if (BWD) {
      const float4 gg = ld4(g + e);
      const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = bn_dx(o[u], gv[u], mu[u], rs[u], sc[u], sh[u], k1[u], k2[u], act, train);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = bn_out(o[u], sc[u], sh[u], act);
      if (res) { const float4 q = ld4(res + e); o[0] += q.x; o[1] += q.y; o[2] += q.z; o[3] += q.w; }
    }
    st4(out + e, make_float4(o[0], o[1], o[2], o[3]));
  }
}

template <int BWD>
__global__ void __launch_bounds__(256) bn_elem_planes_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ res, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ w,
                                                             const float* __restrict__ b, const float* __restrict__ dw,
                                                             const float* __restrict__ db, const double* __restrict__ rsums,
                                                             const double* __restrict__ rcount, float inv_n, int act, int train,
                                                             int C, int HW, float* __restrict__ out) {
  if (BWD == 2) inv_n = (float)(1.0 / *rcount);
  const int plane = blockIdx.x;
  const int c = plane % C;
  float sc, sh;
  bn_coef(mean, rstd, w, b, c, sc, sh);
  const float mu = mean[c], rs = rstd[c];
  float k1, k2;
  bn_k<BWD>(dw, db, rsums, inv_n, c, C, k1, k2);
  const long long base = (long long)plane * HW;
  for (int i = threadIdx.x * 4; i < HW; i += 1024) {
    const float4 v = ld4(x + base + i);
    float4 o;
    if (BWD) {
      const float4 gg = ld4(g + base + i);
      o.x = bn_dx(v.x, gg.x, mu, rs, sc, sh, k1, k2, act, train);
      o.y = bn_dx(v.y, gg.y, mu, rs, sc, sh, k1, k2, act, train);
      o.z = bn_dx(v.z, gg.z, mu, rs, sc, sh, k1, k2, act, train);
      o.w = bn_dx(v.w, gg.w, mu, rs, sc, sh, k1, k2, act, train);
    } else {
      o.x = bn_out(v.x, sc, sh, act); o.y = bn_out(v.y, sc, sh, act); o.z = bn_out(v.z, sc, sh, act); o.w = bn_out(v.w, sc, sh, act);
      if (res) { const float4 q = ld4(res + base + i); o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w; }
    }
    st4(out + base + i, o);
  }
}

// ------------------------------------------------------------------------------------------------------------ reflection pad
__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// forward.  layout 1: grid.x = plane * Ho + oh, threads over ow.  layout 0: grid.x = n * Ho + oh, grid.y = channel block of 64,
// lane = channel, the 4 waves stride over ow.
__global__ void __launch_bounds__(256) reflect_pad_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int P,
                                                              int C, int layout) {
  const int Ho = H + 2 * P, Wo = W + 2 * P;
  const int row = blockIdx.x;
  const int plane = row / Ho, oh = row - plane * Ho;
  const int ih = refl(oh - P, H);
  if (layout == 1) {
    const float* src = x + ((long long)plane * H + ih) * W;
    float* dst = y + (long long)row * Wo;
    for (int ow = threadIdx.x; ow < Wo; ow += 256) dst[ow] = src[refl(ow - P, W)];
  } else {
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    if (c >= C) return;
    const float* src = x + ((long long)plane * H + ih) * W * C;
    float* dst = y + (long long)row * Wo * C;
    for (int ow = threadIdx.x >> 6; ow < Wo; ow += 4) dst[(long long)ow * C + c] = src[(long long)refl(ow - P, W) * C + c];
  }
}

// the (up to three) padded coordinates that read input coordinate i, in the fixed order direct, low mirror, high mirror
__device__ __forceinline__ int refl_sources(int i, int n, int P, int* o) {
  int k = 0;
  o[k++] = i + P;
  if (i >= 1 && i <= P) o[k++] = P - i;
  if (i <= n - 2 && i >= n - 1 - P) o[k++] = P + 2 * (n - 1) - i;
  return k;
}

__global__ void __launch_bounds__(256) reflect_pad_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int H, int W, int P,
                                                              int C, int layout) {
  const int Ho = H + 2 * P, Wo = W + 2 * P;
  const int row = blockIdx.x;
  const int plane = row / H, ih = row - plane * H;
  int rs[3];
  const int nr = refl_sources(ih, H, P, rs);
  if (layout == 1) {
    const float* src = gy + (long long)plane * Ho * Wo;
    float* dst = gx + (long long)row * W;
    for (int iw = threadIdx.x; iw < W; iw += 256) {
      int cs[3];
      const int nc = refl_sources(iw, W, P, cs);
      float s = 0.f;
      for (int a = 0; a < nr; ++a)
        for (int bb = 0; bb < nc; ++bb) s += src[(long long)rs[a] * Wo + cs[bb]];
      dst[iw] = s;
    }
  } else {
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    if (c >= C) return;
    const float* src = gy + (long long)plane * Ho * Wo * C;
    float* dst = gx + (long long)row * W * C;
    for (int iw = threadIdx.x >> 6; iw < W; iw += 4) {
      int cs[3];
      const int nc = refl_sources(iw, W, P, cs);
      float s = 0.f;
      for (int a = 0; a < nr; ++a)
        for (int bb = 0; bb < nc; ++bb) s += src[((long long)rs[a] * Wo + cs[bb]) * C + c];
      dst[(long long)iw * C + c] = s;
    }
  }
}

// -------------------------------------------------------------------------------------------------------- non-local attention
// q [F*HW][ldq] (cols 0..A-1), k / v: the UNPOOLED projections [F*HW][ldk] / [F*HW][ldv]; pooled key j = (ph, pw) of the
// Hp x Wp = H/2 x W/2 (floor) pooled grid: max over rows (2ph)W + 2pw + {0, 1, W, W+1} (that order breaks ties).  o [F*HW][ldo],
// lse [F*HW].
template <int A, int V>
struct NL {
  static constexpr int QT = 4096 / V;             // queries per block (forward, dq)
  static constexpr int TPQ = V / 16;              // threads per query row (each owns 16 value columns: c = j0 + TPQ i)
  static constexpr int KT = V == 256 ? 16 : 64;   // key tile (forward, dq)
  static constexpr int KB = 4096 / V;             // keys per block (dk / dv); TPQ threads per key
  static constexpr int QB = (V == 64 || V == 128) ? 32 : 16;   // query tile (dk / dv)
  static constexpr int AP = A + 1;                // padded LDS rows
};

// The grid's geometry, the one thing the two forms of each kernel below differ in (same NL<A, V> tiles, same thread maps, same
// order of every sum).  rows = F*H*W is the offset of the second half of D.
//   NLGeo<true>, the AE configs' grids: H even, W a power of two, every tile divides HW and Lk = HW/4 exactly.  A key's window is
//     decoded with a shift and a mask where it is used; no query, key or store is masked.
//   NLGeo<false>, any H, W >= 2: the last query tile and the last key tile may be partial.
//     - a query past the frame loads the frame's last row (valid memory, finite numbers), stores nothing, and enters dk / dv with P = 0;
//     - a key past Lk has k = v = 0 in LDS, score -inf in the forward (P = exp(-inf - finite) = 0: tile 0 always holds key 0, so the
//       running maximum is finite from the first tile on and no exp(-inf + inf) is formed) and P = 0 in the backward.
//     Wr[j] is the first row of the window of the tile's key j, -1 past Lk: the one division per key is done once per tile, by one
//     thread per key, not in the element loops.
template <bool EXACT>
struct NLGeo;

template <>
struct NLGeo<true> {
  long long rows;
  int HW, W, wsh;                                 // Wp = 1 << wsh
  static NLGeo make(int F, int H, int W) {
    int wsh = 0;
    while ((1 << wsh) < W / 2) ++wsh;
    return {(long long)F * H * W, H * W, W, wsh};
  }
  __device__ __forceinline__ int tiles(int n, int T) const { return n / T; }
  __device__ __forceinline__ int keys() const { return HW >> 2; }
  __device__ __forceinline__ int qrow(int i) const { return i; }
  __device__ __forceinline__ bool qlive(int) const { return true; }
  __device__ __forceinline__ void windows(int, int, int*) const {}
  // first row of the window of key k0 + j
  __device__ __forceinline__ long long window(const int*, int k0, int j) const {
    const int key = k0 + j;
    return (long long)(2 * (key >> wsh)) * W + 2 * (key & ((1 << wsh) - 1));
  }
  static __device__ __forceinline__ bool klive(long long) { return true; }
};

template <>
struct NLGeo<false> {
  long long rows;
  int HW, W, Wp, Lk;
  static NLGeo make(int F, int H, int W) { return {(long long)F * H * W, H * W, W, W / 2, (H / 2) * (W / 2)}; }
  __device__ __forceinline__ int tiles(int n, int T) const { return (n + T - 1) / T; }
  __device__ __forceinline__ int keys() const { return Lk; }
  __device__ __forceinline__ int qrow(int i) const { return min(i, HW - 1); }
  __device__ __forceinline__ bool qlive(int i) const { return i < HW; }
  // fills Wr for the T keys from k0 on; the threads meet before the first read
  __device__ __forceinline__ void windows(int k0, int T, int* Wr) const {
    if ((int)threadIdx.x < T) {
      const int key = k0 + threadIdx.x, ph = key / Wp;
      Wr[threadIdx.x] = key < Lk ? 2 * ph * W + 2 * (key - ph * Wp) : -1;
    }
    __syncthreads();
  }
  __device__ __forceinline__ int window(const int* Wr, int, int j) const { return Wr[j]; }
  static __device__ __forceinline__ bool klive(int r) { return r >= 0; }
};

// pooled value and the arg-max (0..3, row-major window order, first maximum wins) of element col of the window whose first row is r
__device__ __forceinline__ float pool_at(const float* __restrict__ base, long long ld, long long r, int W, int col, int& am) {
  const float v0 = base[r * ld + col], v1 = base[(r + 1) * ld + col], v2 = base[(r + W) * ld + col], v3 = base[(r + W + 1) * ld + col];
  float m = v0; am = 0;
  if (v1 > m) { m = v1; am = 1; }
  if (v2 > m) { m = v2; am = 2; }
  if (v3 > m) { m = v3; am = 3; }
  return m;
}

// pool_at, 0 (and arg-max 0) for a key past Lk
template <class G, class R>
__device__ __forceinline__ float pool_key(const G& g, const float* __restrict__ base, long long ld, R r, int col, int& am) {
  am = 0;
  return G::klive(r) ? pool_at(base, ld, r, g.W, col, am) : 0.f;
}

template <int A, int V, int KT, class G>
__device__ __forceinline__ void nl_load_kv(const G& g, const float* __restrict__ kf, long long ldk, const float* __restrict__ vf,
                                           long long ldv, int k0, const int* Wr, float* Ks, float* Vs) {
  constexpr int AP = A + 1;
  for (int e = threadIdx.x; e < KT * A; e += 256) {
    const int j = e / A, d = e % A;
    int am;
    Ks[j * AP + d] = pool_key(g, kf, ldk, g.window(Wr, k0, j), d, am);
  }
  for (int e = threadIdx.x; e < KT * V; e += 256) {
    const int j = e / V, c = e % V;
    int am;
    Vs[j * V + c] = pool_key(g, vf, ldv, g.window(Wr, k0, j), c, am);
  }
}

// S[qi][j] = q_qi . k_j for the block's QT x KT tile: mode 0 stores S (-inf at a key past Lk), mode 1 exp(S - lse[qi]) (0 there)
template <int A, int QT, int KT, class G>
__device__ __forceinline__ void nl_scores(const G& g, const float* Qs, const float* Ks, float* Ss, const float* Ls, const int* Wr,
                                          int k0, int mode) {
  constexpr int AP = A + 1;
  for (int e = threadIdx.x; e < QT * KT; e += 256) {
    const int qi = e / KT, j = e % KT;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < A; ++d) s = fmaf(Qs[qi * AP + d], Ks[j * AP + d], s);
    const bool live = G::klive(g.window(Wr, k0, j));
    Ss[qi * (KT + 1) + j] = mode ? (live ? expf(s - Ls[qi]) : 0.f) : (live ? s : -INFINITY);
  }
}

template <int A, int V, bool EXACT>
__global__ void __launch_bounds__(256) nl_attn_fwd_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ k,
                                                          long long ldk, const float* __restrict__ v, long long ldv,
                                                          float* __restrict__ o, long long ldo, float* __restrict__ lse,
                                                          const NLGeo<EXACT> g) {
  using C = NL<A, V>;
  constexpr int QT = C::QT, KT = C::KT, TPQ = C::TPQ, AP = C::AP;
  __shared__ float Qs[QT * AP], Ks[KT * AP], Vs[KT * V], Ss[QT * (KT + 1)];
  __shared__ int Wr[KT];
  const int HW = g.HW, tiles = g.tiles(HW, QT);
  const int f = blockIdx.x / tiles, q0 = (blockIdx.x - f * tiles) * QT;
  const long long fb = (long long)f * HW;
  const int Lk = g.keys();
  for (int e = threadIdx.x; e < QT * A; e += 256) Qs[(e / A) * AP + e % A] = q[(fb + g.qrow(q0 + e / A)) * ldq + e % A];
  const int qi = threadIdx.x / TPQ, j0 = threadIdx.x % TPQ;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float mrun = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += KT) {
    __syncthreads();
    g.windows(k0, KT, Wr);
    nl_load_kv<A, V, KT>(g, k + fb * ldk, ldk, v + fb * ldv, ldv, k0, Wr, Ks, Vs);
    __syncthreads();
    nl_scores<A, QT, KT>(g, Qs, Ks, Ss, nullptr, Wr, k0, 0);
    __syncthreads();
    const float* srow = Ss + qi * (KT + 1);
    float mx = mrun;
    for (int j = 0; j < KT; ++j) mx = fmaxf(mx, srow[j]);
    const float corr = expf(mrun - mx);
    l *= corr;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] *= corr;
    for (int j = 0; j < KT; ++j) {
      const float p = expf(srow[j] - mx);
      l += p;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fmaf(p, Vs[j * V + j0 + TPQ * i], acc[i]);
    }
    mrun = mx;
  }
  if (!g.qlive(q0 + qi)) return;
  const float inv = 1.f / l;
  const long long row = fb + q0 + qi;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[row * ldo + j0 + TPQ * i] = acc[i] * inv;
  if (j0 == 0) lse[row] = mrun + logf(l);
}

// butterfly sum over the TPQ lanes of a query / key group (aligned, contiguous lanes): fixed order, every lane gets the total
template <int TPQ>
__device__ __forceinline__ float group_sum(float s) {
#pragma unroll
  for (int o = TPQ / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// dq, and per query D_i = sum_j Phat_ij dP_ij (= rowsum(dO * O)) and r_i = 1 / sum_j P_ij, saved for the dk / dv kernel
// (D [2][F*H*W]: D, then r).  P_ij = exp(s_ij - lse_i) is recomputed; the rounding of lse scales a whole row by the same 1 + eps,
// and so does an error in D taken from the rounded forward output: neither averages out over the keys, and dq, a sum whose terms
// cancel, showed them (2.1e-5 - 2.5e-5 rel-L2 against float64 over 1024 keys, measured).  So a first sweep over the keys sums
// sum_j P_ij and sum_j P_ij dP_ij in double, and both backward kernels use Phat = P r, whose row sums to 1.
template <int A, int V, bool EXACT>
__global__ void __launch_bounds__(256) nl_attn_dq_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ k,
                                                         long long ldk, const float* __restrict__ v, long long ldv,
                                                         const float* __restrict__ go,
                                                         long long ldgo, const float* __restrict__ lse, float* __restrict__ Dout,
                                                         float* __restrict__ dq, long long lddq, const NLGeo<EXACT> g) {
  using C = NL<A, V>;
  constexpr int QT = C::QT, KT = C::KT, TPQ = C::TPQ, AP = C::AP;
  constexpr int NQ = QT * A / 256;      // dq accumulators per thread (4 at every supported shape: QT A = 1024)
  __shared__ float Qs[QT * AP], Ks[KT * AP], Vs[KT * V], Ss[QT * (KT + 1)], Ls[QT];
  __shared__ int Wr[KT];
  const int HW = g.HW, tiles = g.tiles(HW, QT);
  const int f = blockIdx.x / tiles, q0 = (blockIdx.x - f * tiles) * QT;
  const long long fb = (long long)f * HW;
  const int Lk = g.keys();
  for (int e = threadIdx.x; e < QT * A; e += 256) Qs[(e / A) * AP + e % A] = q[(fb + g.qrow(q0 + e / A)) * ldq + e % A];
  const int qi = threadIdx.x / TPQ, j0 = threadIdx.x % TPQ;
  const bool live = g.qlive(q0 + qi);
  const long long row = fb + g.qrow(q0 + qi);
  float gr[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) gr[i] = go[row * ldgo + j0 + TPQ * i];
  if (j0 == 0) Ls[qi] = lse[row];
  double dacc = 0.0, pacc = 0.0;
  for (int k0 = 0; k0 < Lk; k0 += KT) {
    __syncthreads();
    g.windows(k0, KT, Wr);
    nl_load_kv<A, V, KT>(g, k + fb * ldk, ldk, v + fb * ldv, ldv, k0, Wr, Ks, Vs);
    __syncthreads();
    nl_scores<A, QT, KT>(g, Qs, Ks, Ss, Ls, Wr, k0, 1);      // P
    __syncthreads();
    for (int j = 0; j < KT; ++j) {
      float dp = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) dp = fmaf(gr[i], Vs[j * V + j0 + TPQ * i], dp);
      dp = group_sum<TPQ>(dp);
      const double p = (double)Ss[qi * (KT + 1) + j];
      dacc += p * (double)dp;
      pacc += p;
    }
  }
  const float dsum = (float)(dacc / pacc), rinv = (float)(1.0 / pacc);
  if (j0 == 0 && live) { Dout[row] = dsum; Dout[g.rows + row] = rinv; }
  float acc[NQ];
#pragma unroll
  for (int m = 0; m < NQ; ++m) acc[m] = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += KT) {
    __syncthreads();
    g.windows(k0, KT, Wr);
    nl_load_kv<A, V, KT>(g, k + fb * ldk, ldk, v + fb * ldv, ldv, k0, Wr, Ks, Vs);
    __syncthreads();
    nl_scores<A, QT, KT>(g, Qs, Ks, Ss, Ls, Wr, k0, 1);      // P
    __syncthreads();
    for (int j = 0; j < KT; ++j) {
      float dp = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) dp = fmaf(gr[i], Vs[j * V + j0 + TPQ * i], dp);
      dp = group_sum<TPQ>(dp);
      if (j0 == 0) { float* s = Ss + qi * (KT + 1) + j; *s = (*s * rinv) * (dp - dsum); }       // dS = Phat (dP - D)
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NQ; ++m) {
      const int e = threadIdx.x + 256 * m, qq = e / A, d = e % A;
      float s = acc[m];
      for (int j = 0; j < KT; ++j) s = fmaf(Ss[qq * (KT + 1) + j], Ks[j * AP + d], s);
      acc[m] = s;
    }
  }
#pragma unroll
  for (int m = 0; m < NQ; ++m) {
    const int e = threadIdx.x + 256 * m, qq = e / A, d = e % A;
    if (g.qlive(q0 + qq)) dq[(fb + q0 + qq) * lddq + d] = acc[m];
  }
}

// one value's gradient to the arg-max of its window (first row r), 0 to the other three positions
__device__ __forceinline__ void unpool_store(float* __restrict__ base, long long ld, long long r, int W, int col, int am, float val) {
  base[r * ld + col] = am == 0 ? val : 0.f;
  base[(r + 1) * ld + col] = am == 1 ? val : 0.f;
  base[(r + W) * ld + col] = am == 2 ? val : 0.f;
  base[(r + W + 1) * ld + col] = am == 3 ? val : 0.f;
}

// dk, dv of KB pooled keys, routed to the arg-max of each window (the other three window positions get 0: with the edge kernel
// below every element of the unpooled gradient is written exactly once)
template <int A, int V, bool EXACT>
__global__ void __launch_bounds__(256) nl_attn_dkv_kernel(const float* __restrict__ q, long long ldq, const float* __restrict__ k,
                                                          long long ldk, const float* __restrict__ v, long long ldv,
                                                          const float* __restrict__ go, long long ldgo, const float* __restrict__ lse,
                                                          const float* __restrict__ Din, float* __restrict__ dk, long long lddk,
                                                          float* __restrict__ dv, long long lddv, const NLGeo<EXACT> g) {
  using C = NL<A, V>;
  constexpr int KB = C::KB, QB = C::QB, TPQ = C::TPQ, AP = C::AP;
  constexpr int NK = KB * A / 256;      // dk accumulators per thread (4 at every supported shape: KB A = 1024)
  __shared__ float Ks[KB * AP], Qs[QB * AP], Gs[QB * V], Ps[KB * (QB + 1)], Es[KB * (QB + 1)], Ls[QB], Ds[QB], Rs[QB];
  __shared__ unsigned char Kam[KB * A], Vam[KB * V];
  __shared__ int Wr[KB];
  const int HW = g.HW, W = g.W, tiles = g.tiles(g.keys(), KB);
  const int f = blockIdx.x / tiles, kb0 = (blockIdx.x - f * tiles) * KB;
  const long long fb = (long long)f * HW;
  g.windows(kb0, KB, Wr);
  for (int e = threadIdx.x; e < KB * A; e += 256) {
    int am;
    Ks[(e / A) * AP + e % A] = pool_key(g, k + fb * ldk, ldk, g.window(Wr, kb0, e / A), e % A, am);
    Kam[e] = (unsigned char)am;
  }
  const int jr = threadIdx.x / TPQ, j0 = threadIdx.x % TPQ;
  float vr[16], dvr[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    int am;
    vr[i] = pool_key(g, v + fb * ldv, ldv, g.window(Wr, kb0, jr), j0 + TPQ * i, am);
    Vam[jr * V + j0 + TPQ * i] = (unsigned char)am;
    dvr[i] = 0.f;
  }
  float dkr[NK];
#pragma unroll
  for (int m = 0; m < NK; ++m) dkr[m] = 0.f;
  for (int q0 = 0; q0 < HW; q0 += QB) {
    __syncthreads();
    for (int e = threadIdx.x; e < QB * A; e += 256) Qs[(e / A) * AP + e % A] = q[(fb + g.qrow(q0 + e / A)) * ldq + e % A];
    for (int e = threadIdx.x; e < QB * V; e += 256) Gs[e] = go[(fb + g.qrow(q0 + e / V)) * ldgo + e % V];
    if (threadIdx.x < QB) {
      const long long rw = fb + g.qrow(q0 + (int)threadIdx.x);
      Ls[threadIdx.x] = lse[rw]; Ds[threadIdx.x] = Din[rw];
      Rs[threadIdx.x] = g.qlive(q0 + (int)threadIdx.x) ? Din[g.rows + rw] : 0.f;      // r = 0: a query past the frame has Phat = 0
    }
    __syncthreads();
    for (int e = threadIdx.x; e < KB * QB; e += 256) {
      const int jj = e / QB, qi = e % QB;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < A; ++d) s = fmaf(Qs[qi * AP + d], Ks[jj * AP + d], s);
      Ps[jj * (QB + 1) + qi] = expf(s - Ls[qi]) * Rs[qi];
    }
    __syncthreads();
    for (int qi = 0; qi < QB; ++qi) {
      const float p = Ps[jr * (QB + 1) + qi];
      float dp = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float gg = Gs[qi * V + j0 + TPQ * i];
        dp = fmaf(gg, vr[i], dp);
        dvr[i] = fmaf(p, gg, dvr[i]);
      }
      dp = group_sum<TPQ>(dp);
      if (j0 == 0) Es[jr * (QB + 1) + qi] = p * (dp - Ds[qi]);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NK; ++m) {
      const int e = threadIdx.x + 256 * m, jj = e / A, d = e % A;
      float s = dkr[m];
      for (int qi = 0; qi < QB; ++qi) s = fmaf(Es[jj * (QB + 1) + qi], Qs[qi * AP + d], s);
      dkr[m] = s;
    }
  }
  __syncthreads();
  const auto wv = g.window(Wr, kb0, jr);
  if (g.klive(wv)) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = j0 + TPQ * i;
      unpool_store(dv, lddv, fb + wv, W, c, Vam[jr * V + c], dvr[i]);
    }
  }
#pragma unroll
  for (int m = 0; m < NK; ++m) {
    const int e = threadIdx.x + 256 * m, jj = e / A, d = e % A;
    const auto wk = g.window(Wr, kb0, jj);
    if (g.klive(wk)) unpool_store(dk, lddk, fb + wk, W, d, Kam[e], dkr[m]);
  }
}

// dk = dv = 0 on the rows no window covers: the last line of an odd H (W rows a frame), then the last column of an odd W (the
// corner belongs to the line): n rows a frame.  One block per such row, so with the dk / dv kernel every element is written exactly
// once.
__global__ void __launch_bounds__(64) nlg_attn_edge_kernel(float* __restrict__ dk, long long lddk, float* __restrict__ dv, long long lddv,
                                                           int H, int W, int n, int A, int V) {
  const int line = (H & 1) ? W : 0;
  const int f = blockIdx.x / n, i = blockIdx.x - f * n;
  const long long r = (long long)f * H * W + (i < line ? (long long)(H - 1) * W + i : (long long)(i - line) * W + W - 1);
  for (int c = threadIdx.x; c < A; c += 64) dk[r * lddk + c] = 0.f;
  for (int c = threadIdx.x; c < V; c += 64) dv[r * lddv + c] = 0.f;
}

static inline int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

}  // namespace npvp

using namespace npvp;

// ------------------------------------------------------------------------------------------------------------ C entry points

// BatchNorm: one problem record with one check, one part plan, one launcher per pass.  The six entry points compose them: a fused
// call and its synchronised halves differ in where the count (host / device) and the sums (workspace / caller's buffer) come from.
extern "C" int npvp_bn_workspace_bytes(int C) { return C > 0 && C <= 4096 ? (BN_MAX_PARTS + 1) * 2 * C * (int)sizeof(double) : -1; }

struct BnProblem { long long outer, inner; int C, layout, act; };

static int bn_fail(const char* name, const char* what) {
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: %s", name, what);
  npvp_set_error(msg);
  return NPVP_ERR_ARG;
}
#define BN_REQUIRE(cond, what) do { if (!(cond)) return bn_fail(name, what); } while (0)

// shape, act and the 16-byte alignment of the element buffers a0 | a1 | a2 (null: not one of this call's), under the entry point's name
static int bn_check(const BnProblem& p, const char* name, const void* a0, const void* a1, const void* a2) {
  BN_REQUIRE(p.outer > 0 && p.inner > 0 && p.C > 0, "empty problem");
  BN_REQUIRE(p.layout == 0 || p.layout == 1, "layout 0 (rows [outer][C]) or 1 (planes [N*C][H*W])");
  if (p.layout == 0)
    BN_REQUIRE(p.inner == p.C && p.C % 4 == 0 && p.C <= 1024 && 256 % (p.C / 4) == 0, "layout 0 needs inner == C, C a power of two in [4, 1024]");
  else
    BN_REQUIRE(p.outer % p.C == 0 && p.inner % 4 == 0 && p.inner <= (1ll << 30), "layout 1 needs outer = N*C planes of H*W % 4 == 0");
  BN_REQUIRE(p.act == 0 || p.act == 1, "act 0 (none) or 1 (ReLU)");
  BN_REQUIRE((((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)a2) & 15) == 0, "buffers must be 16-byte aligned");
  return NPVP_OK;
}

// first level of the per-channel sums: P parts of `per` rows (layout 0) or planes of one channel (layout 1) each
struct BnParts { int P; long long per; };
static BnParts bn_parts(const BnProblem& p) {
  const long long n = p.layout == 0 ? p.outer : p.outer / p.C;
  const int blocks = p.layout == 0 ? (p.C + 63) / 64 : p.C;      // grid.x of the part kernel: about 2048 blocks in all
  const int P = clampi(p.layout == 0 ? (n + 255) / 256 : n, 1, clampi(2048 / blocks, 1, BN_MAX_PARTS));
  const long long per = (n + P - 1) / P;
  return {(int)((n + per - 1) / per), per};
}

// The workspace holds `lead` doubles the call keeps in front (npvp_bn_act_bwd: its 2C sums; else 0), then part[P][2][C].  Two rules:
//   parts (npvp_bn_stats, npvp_bn_act_bwd): what this problem's P parts take, no more;
//   whole (npvp_bn_bwd_sums): npvp_bn_workspace_bytes(C) as well, whatever the shape.
static int bn_check_ws(const BnProblem& p, const char* name, long long ws_bytes, int lead, bool whole) {
  const long long need = (lead + (long long)bn_parts(p).P * 2 * p.C) * (long long)sizeof(double);
  BN_REQUIRE(ws_bytes >= need && (!whole || ws_bytes >= npvp_bn_workspace_bytes(p.C)), "workspace too small (npvp_bn_workspace_bytes)");
  return NPVP_OK;
}

// partial sums (MODE 0: x / MODE 1: backward pair) through part -> sums[2][C] (double); MODE 1: and dw / db (float) from them
template <int MODE>
static int bn_sums(const BnProblem& p, const float* x, const float* g, const float* mean, const float* rstd, const float* w,
                    const float* b, double* sums, double* part, float* dw, float* db, hipStream_t stream) {
  const BnParts pp = bn_parts(p);
  if (p.layout == 0)
    NPVP_LAUNCH(bn_part_rows_kernel<MODE>, dim3((p.C + 63) / 64, pp.P), dim3(256), 0, stream, x, g, mean, rstd, w, b, p.act, p.outer, p.C,
                pp.per, part);
  else
    NPVP_LAUNCH(bn_part_planes_kernel<MODE>, dim3(p.C, pp.P), dim3(256), 0, stream, x, g, mean, rstd, w, b, p.act, (int)(p.outer / p.C),
                p.C, (int)p.inner, (int)pp.per, part);
  NPVP_LAUNCH(bn_part_reduce_kernel, dim3(2 * p.C), dim3(64), 0, stream, part, pp.P, p.C, sums);
  if (MODE == 1) NPVP_LAUNCH(bn_bwd_finalize_kernel, dim3((p.C + 255) / 256), dim3(256), 0, stream, sums, p.C, dw, db);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// the elementwise pass.  BWD 0: out = y; 1: out = dx from this call's dw / db and the host's count; 2: dx from sums and *count_dev
template <int BWD>
static int bn_elem(const BnProblem& p, const float* x, const float* g, const float* residual, const float* mean, const float* rstd,
                   const float* w, const float* b, const float* dw, const float* db, const double* sums, const double* count_dev,
                   int train, float* out, hipStream_t stream) {
  const float inv_n = (float)(1.0 / (double)(p.outer * p.inner / p.C));
  if (p.layout == 0)
    NPVP_LAUNCH(bn_elem_rows_kernel<BWD>, dim3(clampi((p.outer * p.C / 4 + 255) / 256, 1, 8192)), dim3(256), 0, stream, x, g, residual, mean,
                rstd, w, b, dw, db, sums, count_dev, inv_n, p.act, train, p.outer, p.C, out);
  else
    NPVP_LAUNCH(bn_elem_planes_kernel<BWD>, dim3((unsigned)p.outer), dim3(256), 0, stream, x, g, residual, mean, rstd, w, b, dw, db, sums,
                count_dev, inv_n, p.act, train, p.C, (int)p.inner, out);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// forward from the sums (null: eval): checks, mean / rstd and running statistics from `count` or *count_dev elements per channel, apply
static int bn_forward(const char* name, const BnProblem& p, const float* x, const float* w, const float* b, const float* residual,
                      const double* sums, double count, const double* count_dev, float eps, float momentum, float* running_mean,
                      float* running_var, float* y, float* mean, float* rstd, hipStream_t stream) {
  BN_REQUIRE(x && w && b && y && mean && rstd, "null buffer");
  if (int rc = bn_check(p, name, x, y, residual)) return rc;
  BN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var together");
  NPVP_LAUNCH(bn_finalize_kernel, dim3((p.C + 255) / 256), dim3(256), 0, stream, sums, count, count_dev, eps, momentum, running_mean,
              running_var, p.C, mean, rstd);
  return bn_elem<0>(p, x, nullptr, residual, mean, rstd, w, b, nullptr, nullptr, nullptr, nullptr, 1, y, stream);
}

extern "C" int npvp_bn_stats(const float* x, long long outer, long long inner, int C, int layout, double* sums, void* workspace,
                             long long ws_bytes, hipStream_t stream) {
  NPVP_CHECK_ARG(x && sums && workspace, "bn_stats: null buffer");
  const BnProblem p{outer, inner, C, layout, 0};
  if (bn_check(p, "bn_stats", x, nullptr, nullptr) || bn_check_ws(p, "bn_stats", ws_bytes, 0, false)) return NPVP_ERR_ARG;
  return bn_sums<0>(p, x, nullptr, nullptr, nullptr, nullptr, nullptr, sums, reinterpret_cast<double*>(workspace), nullptr, nullptr, stream);
}

extern "C" int npvp_bn_act_apply(const float* x, const float* w, const float* b, const float* residual, const double* sums, long long count,
                                 float eps, float momentum, float* running_mean, float* running_var, long long outer, long long inner,
                                 int C, int layout, int act, float* y, float* mean, float* rstd, hipStream_t stream) {
  NPVP_CHECK_ARG(sums ? count >= 1 : (running_mean && running_var), "bn_act_apply: sums + count, or running statistics (eval)");
  return bn_forward("bn_act_apply", {outer, inner, C, layout, act}, x, w, b, residual, sums, (double)count, nullptr, eps, momentum,
                    running_mean, running_var, y, mean, rstd, stream);
}

extern "C" int npvp_bn_act_bwd(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                               long long outer, long long inner, int C, int layout, int act, int train, float* dx, float* dw, float* db,
                               void* workspace, long long ws_bytes, hipStream_t stream) {
  NPVP_CHECK_ARG(g && x && mean && rstd && w && b && dx && dw && db && workspace, "bn_act_bwd: null buffer");
  const BnProblem p{outer, inner, C, layout, act};
  if (bn_check(p, "bn_act_bwd", x, g, dx) || bn_check_ws(p, "bn_act_bwd", ws_bytes, 2 * C, false)) return NPVP_ERR_ARG;
  double* sums = reinterpret_cast<double*>(workspace);
  if (int rc = bn_sums<1>(p, x, g, mean, rstd, w, b, sums, sums + 2 * C, dw, db, stream)) return rc;
  return bn_elem<1>(p, x, g, nullptr, mean, rstd, w, b, dw, db, nullptr, nullptr, train, dx, stream);
}

// ---- synchronised BatchNorm (Lightning's sync_batchnorm=True, ref/train_AutoEncoder_lightning.py:40-42): the two passes above cut at
// the point where the per-channel sums cross the ranks.  With this rank's own sums and count they give the bits of the calls above.

extern "C" int npvp_bn_act_apply_sync(const float* x, const float* w, const float* b, const float* residual, const double* stat, float eps,
                                      float momentum, float* running_mean, float* running_var, long long outer, long long inner, int C,
                                      int layout, int act, float* y, float* mean, float* rstd, hipStream_t stream) {
  NPVP_CHECK_ARG(stat && ((uintptr_t)stat & 7) == 0,
                 "bn_act_apply_sync: null stat / not 8-byte aligned (device [sum x, sum x^2, n], 2C+1 doubles)");
  return bn_forward("bn_act_apply_sync", {outer, inner, C, layout, act}, x, w, b, residual, stat, 0.0, stat + 2 * (long long)C, eps,
                    momentum, running_mean, running_var, y, mean, rstd, stream);
}

extern "C" int npvp_bn_bwd_sums(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                                long long outer, long long inner, int C, int layout, int act, double* sums, float* dw, float* db,
                                void* workspace, long long ws_bytes, hipStream_t stream) {
  NPVP_CHECK_ARG(sums && ((uintptr_t)sums & 7) == 0, "bn_bwd_sums: null sums / not 8-byte aligned (device [sum g', sum g' xhat], 2C doubles)");
  NPVP_CHECK_ARG(g && x && mean && rstd && w && b && dw && db && workspace, "bn_bwd_sums: null buffer");
  const BnProblem p{outer, inner, C, layout, act};
  if (bn_check(p, "bn_bwd_sums", x, g, nullptr) || bn_check_ws(p, "bn_bwd_sums", ws_bytes, 0, true)) return NPVP_ERR_ARG;
  return bn_sums<1>(p, x, g, mean, rstd, w, b, sums, reinterpret_cast<double*>(workspace), dw, db, stream);
}

extern "C" int npvp_bn_act_bwd_apply(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                                     const double* sums, const double* count, long long outer, long long inner, int C, int layout,
                                     int act, float* dx, hipStream_t stream) {
  NPVP_CHECK_ARG(sums && ((uintptr_t)sums & 7) == 0, "bn_act_bwd_apply: null sums / not 8-byte aligned (device [sum g', sum g' xhat], summed)");
  NPVP_CHECK_ARG(count && ((uintptr_t)count & 7) == 0, "bn_act_bwd_apply: null count / not 8-byte aligned (device double: elements per channel)");
  NPVP_CHECK_ARG(g && x && mean && rstd && w && b && dx, "bn_act_bwd_apply: null buffer");
  const BnProblem p{outer, inner, C, layout, act};
  if (int rc = bn_check(p, "bn_act_bwd_apply", x, g, dx)) return rc;
  return bn_elem<2>(p, x, g, nullptr, mean, rstd, w, b, nullptr, nullptr, sums, count, 1, dx, stream);
}
#undef BN_REQUIRE

extern "C" int npvp_reflect_pad(const float* x, float* y, int planes, int H, int W, int C, int P, int layout, int backward,
                                hipStream_t stream) {
  NPVP_CHECK_ARG(x && y && planes > 0 && H > 0 && W > 0 && C > 0, "reflect_pad: empty problem");
  NPVP_CHECK_ARG(P >= 1 && P < H && P < W, "reflect_pad: 1 <= pad < H, W (torch's rule)");
  NPVP_CHECK_ARG(layout == 0 || layout == 1, "reflect_pad: layout 0 (NHWC, planes = N) or 1 (NCHW, planes = N*C)");
  NPVP_CHECK_ARG((long long)planes * (H + 2 * P) < (1ll << 31), "reflect_pad: too many rows");
  const int cb = layout == 0 ? (C + 63) / 64 : 1;
  if (!backward)
    NPVP_LAUNCH(reflect_pad_fwd_kernel, dim3(planes * (H + 2 * P), cb), dim3(256), 0, stream, x, y, H, W, P, C, layout);
  else
    NPVP_LAUNCH(reflect_pad_bwd_kernel, dim3(planes * H, cb), dim3(256), 0, stream, x, y, H, W, P, C, layout);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// ---- non-local attention.  npvp_nonlocal_attn_* take the AE configs' (C, grid) pairs only and launch the exact-tile kernels;
// npvp_nonlocal_attn_grid_* take any H, W >= 2: a config shape launches what npvp_nonlocal_attn_* launch (the same bits), every other
// shape the general kernels.  NPVP_NL_GRID_GENERAL=1 sends the config shapes of the grid entry points to the general kernels too
// (measurements: what the masks cost at a shape both forms can run).
static int nl_fail(bool grid, const char* pass, const char* what) {
  char msg[256];
  snprintf(msg, sizeof(msg), "nonlocal_attn%s%s: %s", grid ? "_grid" : "", pass, what);
  npvp_set_error(msg);
  return NPVP_ERR_ARG;
}
#define NL_REQUIRE(cond, pass, what) do { if (!(cond)) return nl_fail(grid, pass, what); } while (0)

// the (C, grid) pairs of the five AE configs: 64x64 @ C=64, 32x32 @ 128, 16x16 @ 256, 8x8 @ 512, or any H x W of as many cells with
// H even and W a power of two (the tiles of NL<A, V> divide exactly, a key's window decodes with a shift and a mask)
static bool nl_config_shape(int H, int W, int A) {
  return H % 2 == 0 && (W & (W - 1)) == 0 && (long long)H * W == (A == 8 ? 4096 : A == 16 ? 1024 : A == 32 ? 256 : 64);
}

static bool nl_force_general() {
  static const bool on = [] { const char* e = getenv("NPVP_NL_GRID_GENERAL"); return e && e[0] == '1'; }();
  return on;
}

static int nl_check(bool grid, int F, int H, int W, int A, int V) {
  NL_REQUIRE(F > 0 && H >= 2 && W >= 2, "", grid ? "F >= 1, H >= 2, W >= 2" : "H even, W a power of two");
  NL_REQUIRE(grid || (H % 2 == 0 && (W & (W - 1)) == 0), "", "H even, W a power of two");
  NL_REQUIRE(npvp_ae_attn_dims(A, V), "",
             "(attn dim, value dim) must be (8,32), (16,64), (32,128) or (64,256): C = 64..512 of the AE configs");
  NL_REQUIRE(grid || nl_config_shape(H, W, A), "",
             "grid not supported (the AE configs' grids: 64x64 @ C=64, 32x32 @ 128, 16x16 @ 256, 8x8 @ 512)");
  NL_REQUIRE((long long)F * H * W < (1ll << 31), "", "too many rows (F*H*W < 2^31)");
  return NPVP_OK;
}

// MACRO(A, V, exact) for the pair of ae_attn_dims.h that nl_check has let through
#define NL_CASE(a, vv, MACRO, ex) if (A == a) MACRO(a, vv, ex) else
#define NL_DISPATCH(MACRO)                                                                                                         \
  if (exact) {                                                                                                                     \
    NPVP_AE_ATTN_DIMS(NL_CASE, MACRO, true) {}                                                                                     \
  } else {                                                                                                                         \
    NPVP_AE_ATTN_DIMS(NL_CASE, MACRO, false) {}                                                                                    \
  }

// grid: the any-grid entry point (its name in the error texts, its shapes); the other one refuses what is no config shape
static int nl_fwd(bool grid, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                  long long ldo, float* lse, int F, int H, int W, int A, int V, hipStream_t stream) {
  NL_REQUIRE(q && k && v && o && lse, "_fwd", "null buffer");
  if (int rc = nl_check(grid, F, H, W, A, V)) return rc;
  NL_REQUIRE(ldq >= A && ldk >= A && ldv >= V && ldo >= V, "_fwd", "leading dimensions");
  const bool exact = !grid || (nl_config_shape(H, W, A) && !nl_force_general());
  const int QT = 4096 / V;
  const unsigned gq = (unsigned)((long long)F * ((H * W + QT - 1) / QT));
#define NL_FWD(a, vv, ex)                                                                                                          \
  NPVP_LAUNCH((nl_attn_fwd_kernel<a, vv, ex>), dim3(gq), dim3(256), 0, stream, q, ldq, k, ldk, v, ldv, o, ldo, lse,                \
              NLGeo<ex>::make(F, H, W));
  NL_DISPATCH(NL_FWD)
#undef NL_FWD
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

static int nl_bwd(bool grid, const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                  const float* go, long long ldgo, const float* lse, float* D, float* dq, long long lddq, float* dk, long long lddk,
                  float* dv, long long lddv, int F, int H, int W, int A, int V, hipStream_t stream) {
  NL_REQUIRE(q && k && v && go && lse && D && dq && dk && dv, "_bwd", "null buffer");
  if (int rc = nl_check(grid, F, H, W, A, V)) return rc;
  NL_REQUIRE(ldq >= A && ldk >= A && ldv >= V && ldgo >= V && lddq >= A && lddk >= A && lddv >= V, "_bwd", "leading dimensions");
  const bool exact = !grid || (nl_config_shape(H, W, A) && !nl_force_general());
  const int Lk = (H / 2) * (W / 2), T = 4096 / V;                          // T = QT = KB
  const unsigned gq = (unsigned)((long long)F * ((H * W + T - 1) / T)), gk = (unsigned)((long long)F * ((Lk + T - 1) / T));
  const int edge = ((H & 1) ? W : 0) + ((W & 1) ? H - (H & 1) : 0);       // rows of a frame that no window covers
#define NL_BWD(a, vv, ex)                                                                                                          \
  {                                                                                                                                \
    NPVP_LAUNCH((nl_attn_dq_kernel<a, vv, ex>), dim3(gq), dim3(256), 0, stream, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D, dq,      \
                lddq, NLGeo<ex>::make(F, H, W));                                                                                   \
    NPVP_LAUNCH((nl_attn_dkv_kernel<a, vv, ex>), dim3(gk), dim3(256), 0, stream, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D, dk,     \
                lddk, dv, lddv, NLGeo<ex>::make(F, H, W));                                                                         \
  }
  NL_DISPATCH(NL_BWD)
#undef NL_BWD
  if (edge)
    NPVP_LAUNCH(nlg_attn_edge_kernel, dim3((unsigned)((long long)F * edge)), dim3(64), 0, stream, dk, lddk, dv, lddv, H, W, edge, A, V);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_nonlocal_attn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                                      long long ldo, float* lse, int F, int H, int W, int A, int V, hipStream_t stream) {
  return nl_fwd(false, q, ldq, k, ldk, v, ldv, o, ldo, lse, F, H, W, A, V, stream);
}

extern "C" int npvp_nonlocal_attn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                      const float* go, long long ldgo, const float* lse, float* D,
                                      float* dq, long long lddq, float* dk, long long lddk, float* dv, long long lddv, int F, int H, int W,
                                      int A, int V, hipStream_t stream) {
  return nl_bwd(false, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D, dq, lddq, dk, lddk, dv, lddv, F, H, W, A, V, stream);
}

extern "C" int npvp_nonlocal_attn_grid_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                           float* o, long long ldo, float* lse, int F, int H, int W, int A, int V, hipStream_t stream) {
  return nl_fwd(true, q, ldq, k, ldk, v, ldv, o, ldo, lse, F, H, W, A, V, stream);
}

extern "C" int npvp_nonlocal_attn_grid_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                           const float* go, long long ldgo, const float* lse, float* D,
                                           float* dq, long long lddq, float* dk, long long lddk, float* dv, long long lddv, int F, int H,
                                           int W, int A, int V, hipStream_t stream) {
  return nl_bwd(true, q, ldq, k, ldk, v, ldv, go, ldgo, lse, D, dq, lddq, dk, lddk, dv, lddv, F, H, W, A, V, stream);
}
