// The 7 x 7 tail of the frozen decoder on the matrix cores (include/npvp_hip.h, npvp_tail7x7_*): ReflectionPad2d(3) ->
// Conv2d(C_in, C_out, 7) -> Tanh / Sigmoid with C_out <= 4 (the configs: 1 and 3), forward and input gradient, on channels-last
// frames x [F][H][W][C_in] -> NCHW frames y [F][C_out][H][W].  The padding is index math (conv7x7_index.h): no padded copy of x.
//
// Forward.  With N = C_out a direct implicit GEMM would leave the matrix cores idle and read x 49 times; the kernel's COLUMN index
// kw is folded into N instead:
//     Z[(f, h, w')][(kw, co)] = sum_{kh, ci} x[f, refl_H(h + kh - 3), w', ci] w[co, ci, kh, kw]        M = F H W, N = 7 * 4 = 32, K = 7 C_in
//     y[f, co, h, w]          = act( bias[co] + sum_kw Z[(f, h, refl_W(w + kw - 3))][(kw, co)] )
// K is ordered (kh, ci) and C_in % 32 == 0, so a K-step of 32 lies inside one kh: a staged row of A is 128 contiguous bytes of one
// source pixel - conv3x3_f16_kernel's gather with a vertical 7-tap loop and a 32-column tile.  A workgroup owns whole image rows (or,
// for W > 128, a column segment with its halo: tail7x7_plan), so every Z it sums is in its own tile: Z goes to LDS after the K loop,
// then the 7-term shifted sum in a fixed order, bias, activation and planar stores.  Every element of y is written exactly once.
//
// Input gradient.  dz = g act'(y) [F][C_out][H][W] (npvp_act_bwd), then
//     dx[(f, s, t)][ci] = sum_kh sum_{(kw, co)} A[(f, s, t)][kh][(kw, co)] w[co, ci, kh, kw]           M = F H W, N = C_in, K = 7 steps of 32
//     A[(f, s, t)][kh][(kw, co)] = sum over h in adj(s, kh, H), v in adj(t, kw, W) of dz[f, co, h, v]  (tail7x7_adj_src: at most 2 x 2 values)
// the mirror images summed in fp32 before the fp16 split (the kernel is linear: exact algebra); dz is small (C_out planes), its gather
// goes through the caches.  dx is written channels-last, once.
//
// Arithmetic = conv3x3.hip's "f16x3": A scaled by the power of two of its amax slot and split on the fly, B as pre-split scaled planes
// [term][K / 8][N][8], three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation; the LDS stage layout, the register prefetch and
// the one barrier per K-step are conv3x3_f16_kernel's.
//
// The 7 x 7 stem of the frozen ENCODER (npvp_stem7x7_*: thin C_in, wide C_out, planar frames in, channels-last frames out, forward only)
// is the second half of this file; it takes the input gradient's tiles and stages.
#include "gemm.h"
#include "f16_split.h"
#include "conv7x7_index.h"

namespace npvp {

constexpr int T7_BM = 128;
constexpr int T7_KGS_A = T7_BM * 16, T7_A_PLANE = 4 * T7_KGS_A, T7_A_BYTES = 2 * T7_A_PLANE;        // A stage: [term][k-group][128 rows][16 B]
constexpr int T7_ZLD = 33;                                // floats per Z row in LDS (32 + 1: consecutive rows start in consecutive banks)

struct Tail7x7Params {
  const float* x; const _Float16* planes; const float* bias; float* y;
  int H, W, Cin, Cout, act; long long FH;
  const float* x_amax; const float* w_amax;
  Tail7x7Plan plan;
};

// split 8 fp32 values of one row and k-group and store them to the stage (row XOR 4 * k-group: conv3x3_f16_kernel's swizzle)
__device__ __forceinline__ void t7_store_a(char* st, const f32x4 a0, const f32x4 a1, float sa, int g, int row) {
  f16x4 h0, l0, h1, l1;
  split_f16_scaled(a0, sa, h0, l0);
  split_f16_scaled(a1, sa, h1, l1);
  const int off = g * T7_KGS_A + ((row ^ (4 * g)) * 16);
  *reinterpret_cast<f16x8*>(st + off) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  *reinterpret_cast<f16x8*>(st + T7_A_PLANE + off) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void tail7x7_f16_kernel(Tail7x7Params p) {
  constexpr int BN = 32, KGS_B = BN * 16, B_PLANE = 4 * KGS_B, B_BYTES = 2 * B_PLANE, STAGE = T7_A_BYTES + B_BYTES;
  static_assert(T7_BM * T7_ZLD * 4 <= 2 * STAGE, "Z fits in the idle stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  int r0, r1, w0, w1, z0, z1;
  tail7x7_tile(p.plan, blockIdx.x, p.FH, p.W, r0, r1, w0, w1, z0, z1);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 31, h = lane >> 5;
  const float sa = amax_scale(amax_slot_read(p.x_amax)), sb = amax_scale(amax_slot_read(p.w_amax));
  const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
  const int ZW = z1 - z0, nz = (r1 - r0) * ZW;            // Z rows of this tile: (image row, window column), at most 128
  const int spt = Cin >> 5, nk = 7 * spt;                 // K-steps per kh; K-steps

  // A staging: thread (rl, g) stages k-group g of Z rows rl and rl + 64 (rows past nz: the last row, computed and never read)
  const int g = t & 3, rl = t >> 2;
  int ph[2];
  long long fbase[2], pcol[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int zr = rl + 64 * q < nz ? rl + 64 * q : nz - 1;
    const int lr = zr / ZW, gr = r0 + lr, f = gr / H;
    ph[q] = gr - f * H;
    fbase[q] = (long long)f * H;
    pcol[q] = z0 + zr - lr * ZW;
  }
  // B staging: this thread's one 16-byte piece of the K-step's [term][k-group][32 columns]
  const int bc = t & 31, bslab = t >> 5, bs = bslab >> 2, bkg = bslab & 3;
  const long long b_src = (long long)bs * (7ll * Cin * 32) + (bkg * 32 + bc) * 8;
  const int b_dst = T7_A_BYTES + bs * B_PLANE + bkg * KGS_B + bc * 16;

  f32x4 ra[2][2];
  f16x8 rb;
  long long aoff[2] = {0, 0};
  int kh = 0, cs = 0, kt_load = 0;
  auto load = [&]() __attribute__((always_inline)) {
    if (cs == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) aoff[q] = ((fbase[q] + tail7x7_src(ph[q], kh, H)) * W + pcol[q]) * Cin + g * 8;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float* src = p.x + aoff[q] + cs * 32;
      ra[q][0] = *reinterpret_cast<const f32x4*>(src);
      ra[q][1] = *reinterpret_cast<const f32x4*>(src + 4);
    }
    rb = *reinterpret_cast<const f16x8*>(p.planes + (long long)kt_load * (32 * 32) + b_src);
    ++kt_load;
    if (++cs == spt) { cs = 0; ++kh; }
  };
  auto store = [&](char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) t7_store_a(st, ra[q][0], ra[q][1], sa, g, rl + 64 * q);
    *reinterpret_cast<f16x8*>(st + b_dst) = rb;
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  auto compute = [&](const char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kg = 2 * ks + h;
      f16x8 fa[2], fb[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        fa[s] = *reinterpret_cast<const f16x8*>(st + s * T7_A_PLANE + kg * T7_KGS_A + (((wave * 32 + r) ^ (4 * kg)) * 16));
        fb[s] = *reinterpret_cast<const f16x8*>(st + T7_A_BYTES + s * B_PLANE + kg * KGS_B + r * 16);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1], fb[0], acc, 0, 0, 0);        /* smallest terms first, as gemm_f16_body */
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0], fb[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0], fb[0], acc, 0, 0, 0);
    }
  };

  load();
  store(lds);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load();
    compute(lds + cur * STAGE);
    if (more) store(lds + (cur ^ 1) * STAGE);
    __syncthreads();
  }

  // Z to LDS in fp32, back at the operands' scale: accumulator e of lane (r, h) is row (e & 3) + 8 (e >> 2) + 4 h, column r
  float* zs = reinterpret_cast<float*>(lds);
  const float ia = pow2_recip(sa), ib = pow2_recip(sb);
#pragma unroll
  for (int e = 0; e < 16; ++e) zs[(wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * T7_ZLD + r] = acc[e] * ia * ib;
  __syncthreads();

  // y[f, co, h, w] = act(bias[co] + sum_kw Z[(row, refl(w + kw - 3))][(kw, co)]): consecutive threads, consecutive w of one plane
  const int OW = w1 - w0, npix = (r1 - r0) * OW, total = Cout * npix;
  for (int idx = t; idx < total; idx += 256) {
    const int co = idx / npix, pix = idx - co * npix, lr = pix / OW, w = w0 + pix - lr * OW;
    const int gr = r0 + lr, f = gr / H, hh = gr - f * H;
    float v = p.bias[co];
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) v += zs[(lr * ZW + tail7x7_src(w, kw, W) - z0) * T7_ZLD + kw * 4 + co];
    p.y[(((long long)f * Cout + co) * H + hh) * W + w] = ae_act(v, p.act);
  }
}

// What the two 128 x BN implicit GEMMs below share (the tail's input gradient and the encoder's stem; only their A gather, their K-step
// count and their epilogue differ).  BN = 64: 4 waves as 2 x 2, each 64 rows x 32 columns; BN = 32: 4 waves as 4 x 1, each 32 x 32.  A
// stage is the A part t7_store_a fills, then B [term][k-group][BN columns][16 B]; B comes from planes [term][K / 8][N][8].
template <int BN>
struct T7Wide {
  static_assert(BN == 32 || BN == 64, "32 or 64 columns");
  static constexpr int WN = BN / 32, TM = WN;
  static constexpr int KGS_B = BN * 16, B_PLANE = 4 * KGS_B, B_BYTES = 2 * B_PLANE, STAGE = T7_A_BYTES + B_BYTES;
  static constexpr int NB = (8 * BN) / 256;              // 16-byte pieces of a B tile per thread

  // piece i = t + 256 j of a K-step's [term][k-group][column] pieces: its place in the planes (plane_halves = K N halves per term, the
  // tile's columns from n0; a K-step further on is 32 N halves further) and in the stage
  static __device__ __forceinline__ void b_pieces(int t, long long plane_halves, int N, int n0, long long (&src)[NB], int (&dst)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int i = t + 256 * j, c = i % BN, slab = i / BN, s = slab >> 2, kg = slab & 3;
      src[j] = (long long)s * plane_halves + ((long long)kg * N + n0 + c) * 8;
      dst[j] = T7_A_BYTES + s * B_PLANE + kg * KGS_B + c * 16;
    }
  }
  static __device__ __forceinline__ void b_load(const _Float16* kstep, const long long (&src)[NB], f16x8 (&rb)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = *reinterpret_cast<const f16x8*>(kstep + src[j]);
  }
  static __device__ __forceinline__ void b_store(char* st, const int (&dst)[NB], const f16x8 (&rb)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<f16x8*>(st + dst[j]) = rb[j];
  }

  // one K-step of 32 out of a stage, wave (wm, wn), lane (r, h): three MFMAs per product, smallest terms first, as gemm_f16_body
  static __device__ __forceinline__ void compute(const char* st, f32x16 (&acc)[TM], int wm, int wn, int r, int h) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kg = 2 * ks + h;
      f16x8 fa[2][TM], fb[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[s][i] = *reinterpret_cast<const f16x8*>(st + s * T7_A_PLANE + kg * T7_KGS_A + (((wm * TM * 32 + i * 32 + r) ^ (4 * kg)) * 16));
        fb[s] = *reinterpret_cast<const f16x8*>(st + T7_A_BYTES + s * B_PLANE + kg * KGS_B + (wn * 32 + r) * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][i], fb[0], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[1], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[0], acc[i], 0, 0, 0);
      }
    }
  }

  // the K loop over two stages: K-step kt + 1 travels global -> registers (load) while kt is multiplied, and is split and stored to the
  // other stage afterwards (store); one barrier per K-step.  The stages are idle when it returns.
  template <class Load, class Store>
  static __device__ __forceinline__ void run(char* lds, int nk, f32x16 (&acc)[TM], int wm, int wn, int r, int h, Load& load, Store& store) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    load();
    store(lds);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      const bool more = kt + 1 < nk;
      if (more) load();
      compute(lds + cur * STAGE, acc, wm, wn, r, h);
      if (more) store(lds + (cur ^ 1) * STAGE);
      __syncthreads();
    }
  }
};

struct Tail7x7DgradParams {
  const float* dz; const _Float16* planes; float* dx;
  int H, W, Cin, Cout; long long M;
  const float* dz_amax; const float* w_amax;
  Conv3x3Plan plan;
};

template <int BN>
__global__ __launch_bounds__(256, 2) void tail7x7_dgrad_f16_kernel(Tail7x7DgradParams p) {
  using T = T7Wide<BN>;
  constexpr int WN = T::WN, TM = T::TM, NB = T::NB, STAGE = T::STAGE;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  int m0, m1, n0, n1;
  conv3x3_tile(p.plan, blockIdx.x, p.M, m0, m1, n0, n1);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave / WN, wn = wave % WN, r = lane & 31, h = lane >> 5;
  // a staged value sums up to four dz: the scale of 4 * amax keeps the sum inside fp16's range
  const float sa = amax_scale(4.f * amax_slot_read(p.dz_amax)), sb = amax_scale(amax_slot_read(p.w_amax));
  const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout, HW = H * W;

  // A staging: thread (rl, g) builds k-group g = (kw = 2 g, 2 g + 1) x (co = 0..3) of rows rl and rl + 64 (rows past M: the last row)
  const int g = t & 3, rl = t >> 2;
  int ps[2], v0[2][2], v1[2][2];
  long long fb0[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long m = (long long)m0 + rl + 64 * q < p.M ? (long long)m0 + rl + 64 * q : p.M - 1;
    const int f = (int)(m / HW), rem = (int)(m - (long long)f * HW);
    ps[q] = rem / W;
    const int pt = rem - ps[q] * W;
    fb0[q] = (long long)f * Cout * HW;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kw = 2 * g + j;                          // kw = 7 is the padding of K to 32: zeros
      v0[q][j] = kw < 7 ? tail7x7_adj_src(pt, kw, W, 0) : -1;
      v1[q][j] = kw < 7 ? tail7x7_adj_src(pt, kw, W, 1) : -1;
    }
  }
  long long b_src[NB];
  int b_dst[NB];
  T::b_pieces(t, 224ll * Cin, Cin, n0, b_src, b_dst);
  const long long b_step = 32ll * Cin;                   // halves per K-step (one kh): four k-groups of [Cin][8]

  f32x4 ra[2][2];
  f16x8 rb[NB];
  int kh = 0;
  auto load = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int h0 = tail7x7_adj_src(ps[q], kh, H, 0), h1 = tail7x7_adj_src(ps[q], kh, H, 1);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int co = 0; co < 4; ++co) {
          float v = 0.f;
          if (co < Cout) {
            const float* pl = p.dz + fb0[q] + (long long)co * HW;
            if (h0 >= 0) {
              if (v0[q][j] >= 0) v += pl[h0 * W + v0[q][j]];
              if (v1[q][j] >= 0) v += pl[h0 * W + v1[q][j]];
            }
            if (h1 >= 0) {
              if (v0[q][j] >= 0) v += pl[h1 * W + v0[q][j]];
              if (v1[q][j] >= 0) v += pl[h1 * W + v1[q][j]];
            }
          }
          ra[q][j][co] = v;
        }
    }
    T::b_load(p.planes + (long long)kh * b_step, b_src, rb);
    ++kh;
  };
  auto store = [&](char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) t7_store_a(st, ra[q][0], ra[q][1], sa, g, rl + 64 * q);
    T::b_store(st, b_dst, rb);
  };

  f32x16 acc[TM];
  T::run(lds, 7, acc, wm, wn, r, h, load, store);

  const float ia = pow2_recip(sa), ib = pow2_recip(sb);
  const int col = n0 + wn * 32 + r;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const long long m = (long long)m0 + wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (m < m1) p.dx[m * Cin + col] = acc[i][e] * ia * ib;
    }
}

// w [Cout][Cin][7][7] -> forward planes [term][7 Cin / 8][32][8 over k], k = kh * Cin + ci, column n = kw * 4 + co (zero for co >= Cout
// and for kw = 7), scaled by the weight's amax slot and split as conv3x3_planes_kernel splits its own
__global__ __launch_bounds__(256) void tail7x7_planes_kernel(const float* __restrict__ w, int Cin, int Cout, _Float16* __restrict__ out,
                                                             const float* __restrict__ amax) {
  const long long slots = 7ll * Cin * 4, plane = 7ll * Cin * 32;
  const float s = amax_scale(amax_slot_read(amax));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i & 31), kb = (int)(i >> 5), k0 = kb * 8, kh = k0 / Cin, ci = k0 - kh * Cin, kw = n >> 2, co = n & 3;
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (co < Cout && kw < 7) ? w[(((long long)co * Cin + ci + e) * 7 + kh) * 7 + kw] * s : 0.f;
      hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]);
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = hi;
    *reinterpret_cast<f16x8*>(out + plane + i * 8) = lo;
  }
}

// the same weight -> the input gradient's planes [term][7 * 4 k-groups][Cin][8 over k], k = kh * 32 + kw * 4 + co, column n = ci
__global__ __launch_bounds__(256) void tail7x7_dgrad_planes_kernel(const float* __restrict__ w, int Cin, int Cout, _Float16* __restrict__ out,
                                                                   const float* __restrict__ amax) {
  const long long slots = 28ll * Cin, plane = 224ll * Cin;
  const float s = amax_scale(amax_slot_read(amax));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin), kb = (int)(i / Cin), kh = kb >> 2, kg = kb & 3;
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kk = kg * 8 + e, kw = kk >> 2, co = kk & 3;
      const float x = (co < Cout && kw < 7) ? w[(((long long)co * Cin + ci) * 7 + kh) * 7 + kw] * s : 0.f;
      hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]);
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = hi;
    *reinterpret_cast<f16x8*>(out + plane + i * 8) = lo;
  }
}

__global__ __launch_bounds__(256) void tail7x7_zero_slot_kernel(float* slot) {
  for (int i = threadIdx.x; i < AMAX_WORDS * AMAX_STRIDE; i += 256) slot[i] = 0.f;
}

// ---- The 7 x 7 stem of the frozen encoder (npvp_stem7x7_*): ReflectionPad2d(3) -> Conv2d(C_in <= 4, C_out, 7) -> none / ReLU, forward
// only, on PLANAR frames x [F][C_in][H][W] (what the data path hands the encoder) -> channels-last y [F][H][W][C_out]:
//     C[M = F H W][N = C_out] = A[M][K] B[K][N],   A[m][k] = x[f, ci, refl_H(h + kh - 3), refl_W(w + kw - 3)],  (kh, kw, ci) = stem7x7_k(k)
// the input gradient's shape with the roles exchanged (thin K, wide N), so its tiles (tail7x7_dgrad_plan over (M, C_out)), stages,
// t7_store_a and barrier are taken over; K is dense, 49 C_in padded to a multiple of 32 (2 / 4 / 5 / 7 K-steps).  The gather is scalar
// loads through the caches (x is 1 / C_out-th of the output's size); the reflected coordinates are computed per element, nothing is
// tabulated.  The output store is the kernel's floor: the tile goes through LDS (idle after the loop) and leaves as 16-byte stores, a
// wave writing four whole 256-byte rows (BN = 64); the bound of the stored values goes to y_amax.  Written exactly once, no atomics on y.
struct Stem7x7Params {
  const float* x; const _Float16* planes; const float* bias; float* y;
  int H, W, Cout, act; long long M;
  const float* x_amax; const float* w_amax; float* y_amax;
  Conv3x3Plan plan;
};

template <int CIN, int BN>
__global__ __launch_bounds__(256, 2) void stem7x7_f16_kernel(Stem7x7Params p) {
  static_assert(CIN >= 1 && CIN <= 4, "1 to 4 input channels");
  using T = T7Wide<BN>;
  constexpr int WN = T::WN, TM = T::TM, NB = T::NB, STAGE = T::STAGE;
  constexpr int KP = (49 * CIN + 31) / 32 * 32, NK = KP / 32;
  constexpr int YLD = BN + 4;                            // floats per tile row in LDS: 16-byte aligned rows, shifted by four banks
  static_assert(T7_BM * YLD * 4 + 16 <= 2 * STAGE, "the output tile and the amax scratch fit in the idle stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  int m0, m1, n0, n1;
  conv3x3_tile(p.plan, blockIdx.x, p.M, m0, m1, n0, n1);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave / WN, wn = wave % WN, r = lane & 31, h = lane >> 5;
  const float sa = amax_scale(amax_slot_read(p.x_amax)), sb = amax_scale(amax_slot_read(p.w_amax));
  const unsigned int cpeek = amax_peek_block(p.y_amax);
  const int H = p.H, W = p.W, Cout = p.Cout, HW = H * W;

  // A staging: thread (rl, g) gathers k-group g (eight consecutive k) of rows rl and rl + 64 (rows past M: the last row)
  const int g = t & 3, rl = t >> 2;
  int ph[2], pw[2];
  long long fbase[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long m = (long long)m0 + rl + 64 * q < p.M ? (long long)m0 + rl + 64 * q : p.M - 1;
    const int f = (int)(m / HW), rem = (int)(m - (long long)f * HW);
    ph[q] = rem / W; pw[q] = rem - ph[q] * W;
    fbase[q] = (long long)f * CIN * HW;
  }
  long long b_src[NB];
  int b_dst[NB];
  T::b_pieces(t, (long long)KP * Cout, Cout, n0, b_src, b_dst);
  const long long b_step = 32ll * Cout;                 // halves per K-step: four k-groups of [Cout][8]

  f32x4 ra[2][2];
  f16x8 rb[NB];
  int kt_load = 0;
  auto load = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int kh, kw, ci;
      const bool tap = stem7x7_k(CIN, kt_load * 32 + g * 8 + e, kh, kw, ci);      // (false: the zero padding of K)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float v = 0.f;
        if (tap) v = p.x[fbase[q] + (long long)(ci * H + tail7x7_src(ph[q], kh, H)) * W + tail7x7_src(pw[q], kw, W)];
        ra[q][e >> 2][e & 3] = v;
      }
    }
    T::b_load(p.planes + (long long)kt_load * b_step, b_src, rb);
    ++kt_load;
  };
  auto store = [&](char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) t7_store_a(st, ra[q][0], ra[q][1], sa, g, rl + 64 * q);
    T::b_store(st, b_dst, rb);
  };

  f32x16 acc[TM];
  T::run(lds, NK, acc, wm, wn, r, h, load, store);

  // epilogue: back to the operands' scale, + bias, activation, the tile to LDS in the accumulator layout (accumulator e of lane (r, h)
  // is row (e & 3) + 8 (e >> 2) + 4 h, column r), then out in rows: 16 bytes per thread, consecutive threads along a row of y
  float* ys = reinterpret_cast<float*>(lds);
  const float ia = pow2_recip(sa), ib = pow2_recip(sb);
  const float b = p.bias[n0 + wn * 32 + r];
  const int nrows = m1 - m0;
  float cmax = 0.f;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = ae_act(acc[i][e] * ia * ib + b, p.act);
      ys[row * YLD + wn * 32 + r] = v;
      if (row < nrows) cmax = fmaxf(cmax, fabsf(v));
    }
  __syncthreads();
  constexpr int C4 = BN / 4;
  for (int idx = t; idx < T7_BM * C4; idx += 256) {
    const int row = idx / C4, c4 = idx - row * C4;
    if (row < nrows)
      *reinterpret_cast<f32x4*>(p.y + ((long long)m0 + row) * Cout + n0 + c4 * 4) = *reinterpret_cast<const f32x4*>(ys + row * YLD + c4 * 4);
  }
  amax_slot_commit_block(p.y_amax, cmax, reinterpret_cast<float*>(lds + 2 * STAGE - 16), cpeek);       // (behind the tile: nobody reads there)
}

// w [Cout][Cin][7][7] -> the stem's planes [term][K_pad / 8][Cout][8 over k], k by stem7x7_k (zero for the padding of K), scaled by the
// weight's amax slot and split as conv3x3_planes_kernel splits its own
__global__ __launch_bounds__(256) void stem7x7_planes_kernel(const float* __restrict__ w, int Cin, int Cout, _Float16* __restrict__ out,
                                                             const float* __restrict__ amax) {
  const long long plane = (long long)stem7x7_kpad(Cin) * Cout, slots = plane / 8;
  const float s = amax_scale(amax_slot_read(amax));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i % Cout), kb = (int)(i / Cout);
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int kh, kw, ci;
      const float x = stem7x7_k(Cin, kb * 8 + e, kh, kw, ci) ? w[(((long long)n * Cin + ci) * 7 + kh) * 7 + kw] * s : 0.f;
      hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]);
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = hi;
    *reinterpret_cast<f16x8*>(out + plane + i * 8) = lo;
  }
}

}  // namespace npvp

using namespace npvp;

// the shape limits, stated once
static bool tail7x7_channels_ok(int C_in, int C_out) { return C_in > 0 && C_in % 32 == 0 && C_in <= 4096 && C_out >= 1 && C_out <= 4; }

static bool tail7x7_shape_ok(int F, int H, int W, int C_in, int C_out) {
  return F > 0 && H >= 4 && W >= 4 && tail7x7_channels_ok(C_in, C_out) && (long long)F * H * W < (1ll << 31);
}

#define TAIL7X7_CHANNELS_MSG "C_in a multiple of 32 up to 4096, 1 <= C_out <= 4"
#define TAIL7X7_SHAPE_MSG "F >= 1, H, W >= 4 (reflection by 3), " TAIL7X7_CHANNELS_MSG ", F * H * W below 2^31"
#define TAIL7X7_ALIGNED(p) (((uintptr_t)(p) % 16) == 0)

extern "C" int npvp_tail7x7_src(int c, int tap, int extent) {
  if (tap < 0 || tap > 6 || extent < 4 || c < 0 || c >= extent) return -2;
  return tail7x7_src(c, tap, extent);
}

extern "C" int npvp_tail7x7_adj_src(int s, int tap, int extent, int which) {
  if (tap < 0 || tap > 6 || extent < 4 || s < 0 || s >= extent || (which != 0 && which != 1)) return -2;
  return tail7x7_adj_src(s, tap, extent, which);
}

extern "C" long long npvp_tail7x7_planes_bytes(int C_in, int C_out) {
  if (!tail7x7_channels_ok(C_in, C_out)) return -1;
  return 2ll * 7 * C_in * 32 * 2;
}

extern "C" int npvp_tail7x7_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "tail7x7_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(tail7x7_channels_ok(C_in, C_out), "tail7x7_planes: " TAIL7X7_CHANNELS_MSG);
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(w) && TAIL7X7_ALIGNED(planes), "tail7x7_planes: w and planes must be 16-byte aligned");
  NPVP_LAUNCH(tail7x7_zero_slot_kernel, dim3(1), dim3(256), 0, stream, w_amax);          // (a kernel, not a memset node: see gemm_f16.hip)
  NPVP_CHECK_LAUNCH();
  const int rc = npvp_amax(w, C_out, 49ll * C_in, 49ll * C_in, w_amax, stream);
  if (rc != NPVP_OK) return rc;
  const long long slots = 7ll * C_in * 4;
  NPVP_LAUNCH(tail7x7_planes_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, w, C_in, C_out, (_Float16*)planes,
              (const float*)w_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_dgrad_planes(const float* w, int C_in, int C_out, void* planes, const float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "tail7x7_dgrad_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(tail7x7_channels_ok(C_in, C_out), "tail7x7_dgrad_planes: " TAIL7X7_CHANNELS_MSG);
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(w) && TAIL7X7_ALIGNED(planes), "tail7x7_dgrad_planes: w and planes must be 16-byte aligned");
  const long long slots = 28ll * C_in;
  NPVP_LAUNCH(tail7x7_dgrad_planes_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, w, C_in, C_out, (_Float16*)planes,
              w_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_route(int F, int H, int W, int C_in, int C_out, int* out8) {
  NPVP_CHECK_ARG(out8 && tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7: " TAIL7X7_SHAPE_MSG);
  const Tail7x7Plan p = tail7x7_plan((long long)F * H, W);
  out8[0] = p.rows; out8[1] = p.segs; out8[2] = p.seg_cols; out8[3] = p.tiles_r; out8[4] = p.grid; out8[5] = T7_BM; out8[6] = 32;
  out8[7] = 7 * (C_in / 32);
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_tile(int F, int H, int W, int C_in, int C_out, int block, int* out6) {
  NPVP_CHECK_ARG(out6 && tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7: " TAIL7X7_SHAPE_MSG);
  const Tail7x7Plan p = tail7x7_plan((long long)F * H, W);
  NPVP_CHECK_ARG(block >= 0 && block < p.grid, "tail7x7_tile: block outside the plan's grid");
  tail7x7_tile(p, block, (long long)F * H, W, out6[0], out6[1], out6[2], out6[3], out6[4], out6[5]);
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_dgrad_route(int F, int H, int W, int C_in, int C_out, int* out6) {
  NPVP_CHECK_ARG(out6 && tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7_dgrad: " TAIL7X7_SHAPE_MSG);
  const Conv3x3Plan p = tail7x7_dgrad_plan((long long)F * H * W, C_in);
  out6[0] = p.variant; out6[1] = p.bm; out6[2] = p.bn; out6[3] = p.tiles_m; out6[4] = p.tiles_n; out6[5] = p.grid;
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_dgrad_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4) {
  NPVP_CHECK_ARG(out4 && tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7_dgrad: " TAIL7X7_SHAPE_MSG);
  const long long M = (long long)F * H * W;
  const Conv3x3Plan p = tail7x7_dgrad_plan(M, C_in);
  NPVP_CHECK_ARG(block >= 0 && block < p.grid, "tail7x7_dgrad_tile: block outside the plan's grid");
  conv3x3_tile(p, block, M, out4[0], out4[1], out4[2], out4[3]);
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in, int C_out,
                                int act, const float* x_amax, const float* w_amax, void* workspace, long long ws_bytes,
                                hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(x && planes && bias && y && x_amax && w_amax, "tail7x7: x, planes, bias, y, x_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7: " TAIL7X7_SHAPE_MSG);
  NPVP_CHECK_ARG(act == 0 || act == 2 || act == 3, "tail7x7: act 0 (none), 2 (tanh) or 3 (sigmoid)");
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(x) && TAIL7X7_ALIGNED(planes) && TAIL7X7_ALIGNED(y), "tail7x7: x, planes and y must be 16-byte aligned");
  Tail7x7Params p;
  p.x = x; p.planes = (const _Float16*)planes; p.bias = bias; p.y = y;
  p.H = H; p.W = W; p.Cin = C_in; p.Cout = C_out; p.act = act; p.FH = (long long)F * H;
  p.x_amax = x_amax; p.w_amax = w_amax;
  p.plan = tail7x7_plan(p.FH, W);
  NPVP_LAUNCH(tail7x7_f16_kernel, dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_tail7x7_dgrad_f16(const float* dz, const void* planes, float* dx, int F, int H, int W, int C_in, int C_out,
                                      const float* dz_amax, const float* w_amax, void* workspace, long long ws_bytes,
                                      hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(dz && planes && dx && dz_amax && w_amax, "tail7x7_dgrad: dz, planes, dx, dz_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(tail7x7_shape_ok(F, H, W, C_in, C_out), "tail7x7_dgrad: " TAIL7X7_SHAPE_MSG);
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(dz) && TAIL7X7_ALIGNED(planes) && TAIL7X7_ALIGNED(dx),
                 "tail7x7_dgrad: dz, planes and dx must be 16-byte aligned");
  Tail7x7DgradParams p;
  p.dz = dz; p.planes = (const _Float16*)planes; p.dx = dx;
  p.H = H; p.W = W; p.Cin = C_in; p.Cout = C_out; p.M = (long long)F * H * W;
  p.dz_amax = dz_amax; p.w_amax = w_amax;
  p.plan = tail7x7_dgrad_plan(p.M, C_in);
  if (p.plan.variant == 1) NPVP_LAUNCH((tail7x7_dgrad_f16_kernel<64>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  else NPVP_LAUNCH((tail7x7_dgrad_f16_kernel<32>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// ---- the encoder's stem: the shape limits, stated once
static bool stem7x7_channels_ok(int C_in, int C_out) { return C_in >= 1 && C_in <= 4 && C_out > 0 && C_out % 32 == 0 && C_out <= 4096; }

static bool stem7x7_shape_ok(int F, int H, int W, int C_in, int C_out) {
  return F > 0 && H >= 4 && W >= 4 && stem7x7_channels_ok(C_in, C_out) && (long long)F * H * W < (1ll << 31);
}

#define STEM7X7_CHANNELS_MSG "1 <= C_in <= 4, C_out a multiple of 32 up to 4096"
#define STEM7X7_SHAPE_MSG "F >= 1, H, W >= 4 (reflection by 3), " STEM7X7_CHANNELS_MSG ", F * H * W below 2^31"

extern "C" int npvp_stem7x7_k(int C_in, int k, int* out3) {
  if (!out3 || C_in < 1 || C_in > 4 || k < 0 || k >= stem7x7_kpad(C_in)) return -2;
  int kh, kw, ci;
  if (!stem7x7_k(C_in, k, kh, kw, ci)) { out3[0] = out3[1] = out3[2] = -1; return 1; }
  out3[0] = kh; out3[1] = kw; out3[2] = ci;
  return 0;
}

extern "C" long long npvp_stem7x7_planes_bytes(int C_in, int C_out) {
  if (!stem7x7_channels_ok(C_in, C_out)) return -1;
  return 2ll * stem7x7_kpad(C_in) * C_out * 2;
}

extern "C" int npvp_stem7x7_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "stem7x7_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(stem7x7_channels_ok(C_in, C_out), "stem7x7_planes: " STEM7X7_CHANNELS_MSG);
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(w) && TAIL7X7_ALIGNED(planes), "stem7x7_planes: w and planes must be 16-byte aligned");
  NPVP_LAUNCH(tail7x7_zero_slot_kernel, dim3(1), dim3(256), 0, stream, w_amax);          // (a kernel, not a memset node: see gemm_f16.hip)
  NPVP_CHECK_LAUNCH();
  const long long n = 49ll * C_in * C_out;               // (49 C_in is no multiple of 4 for C_in < 4; C_out % 32 == 0 makes the whole one)
  const int rc = npvp_amax(w, 1, n, n, w_amax, stream);
  if (rc != NPVP_OK) return rc;
  const long long slots = (long long)stem7x7_kpad(C_in) * C_out / 8;
  NPVP_LAUNCH(stem7x7_planes_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, w, C_in, C_out, (_Float16*)planes,
              (const float*)w_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_stem7x7_route(int F, int H, int W, int C_in, int C_out, int* out7) {
  NPVP_CHECK_ARG(out7 && stem7x7_shape_ok(F, H, W, C_in, C_out), "stem7x7: " STEM7X7_SHAPE_MSG);
  const Conv3x3Plan p = tail7x7_dgrad_plan((long long)F * H * W, C_out);
  out7[0] = p.variant; out7[1] = p.bm; out7[2] = p.bn; out7[3] = p.tiles_m; out7[4] = p.tiles_n; out7[5] = p.grid;
  out7[6] = stem7x7_kpad(C_in) / 32;
  return NPVP_OK;
}

extern "C" int npvp_stem7x7_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4) {
  NPVP_CHECK_ARG(out4 && stem7x7_shape_ok(F, H, W, C_in, C_out), "stem7x7: " STEM7X7_SHAPE_MSG);
  const long long M = (long long)F * H * W;
  const Conv3x3Plan p = tail7x7_dgrad_plan(M, C_out);
  NPVP_CHECK_ARG(block >= 0 && block < p.grid, "stem7x7_tile: block outside the plan's grid");
  conv3x3_tile(p, block, M, out4[0], out4[1], out4[2], out4[3]);
  return NPVP_OK;
}

template <int CIN>
static void stem7x7_launch(const Stem7x7Params& p, hipStream_t stream) {
  if (p.plan.variant == 1) NPVP_LAUNCH((stem7x7_f16_kernel<CIN, 64>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  else NPVP_LAUNCH((stem7x7_f16_kernel<CIN, 32>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
}

extern "C" int npvp_stem7x7_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in, int C_out,
                                int act, const float* x_amax, const float* w_amax, float* y_amax, void* workspace, long long ws_bytes,
                                hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(x && planes && bias && y && x_amax && w_amax, "stem7x7: x, planes, bias, y, x_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(stem7x7_shape_ok(F, H, W, C_in, C_out), "stem7x7: " STEM7X7_SHAPE_MSG);
  NPVP_CHECK_ARG(act == 0 || act == 1, "stem7x7: act 0 (none) or 1 (ReLU)");
  NPVP_CHECK_ARG(TAIL7X7_ALIGNED(planes) && TAIL7X7_ALIGNED(y), "stem7x7: planes and y must be 16-byte aligned");
  Stem7x7Params p;
  p.x = x; p.planes = (const _Float16*)planes; p.bias = bias; p.y = y;
  p.H = H; p.W = W; p.Cout = C_out; p.act = act; p.M = (long long)F * H * W;
  p.x_amax = x_amax; p.w_amax = w_amax; p.y_amax = y_amax;
  p.plan = tail7x7_dgrad_plan(p.M, C_out);
  if (C_in == 1) stem7x7_launch<1>(p, stream);
  else if (C_in == 2) stem7x7_launch<2>(p, stream);
  else if (C_in == 3) stem7x7_launch<3>(p, stream);
  else stem7x7_launch<4>(p, stream);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
