// 3 x 3 stride-1 "same" convolution of the frozen encoder as an implicit GEMM on the matrix cores (forward only; include/npvp_hip.h,
// npvp_conv3x3_*): the spatial_conv of every Factorized3DConvAttn (zero padding) and the two convolutions of every ResnetBlock
// (ReflectionPad2d(1)), BatchNorm folded into the weights, on channels-last frames x [F][H][W][C_in] -> y [F][H][W][C_out].
//
//     C[M = F H W][N = C_out] = A[M][K = 9 C_in] B[K][N],   A[m][(kh, kw, ci)] = x[f, src(h, kh), src(w, kw), ci]   (gathered, never stored)
//
// Arithmetic = gemm_f16.hip's "f16x3": A is scaled by the power of two of its amax slot and split on the fly (split_f16_scaled), B comes as
// pre-split scaled planes [term][K/8][N][8] (built once: the pair is frozen), three v_mfma_f32_32x32x16_f16 per product, fp32 accumulate.
// K is ordered (kh, kw, ci) and C_in % 64 == 0, so a K-step of 32 lies inside ONE tap: a staged row of A is 128 contiguous bytes of one
// source pixel, or zeros (conv3x3_src of conv3x3_index.h: the padding rule is index math, there is no padded copy of x).
//
// Layout: 128 x 128 (C_out % 128 == 0) or 128 x 64 output tiles, 4 waves as 2 x 2, each 64 x 64 (64 x 32) of 32 x 32 accumulators.
// K-step 32 = four k-groups of 8.  LDS stage = A [term][k-group][128 rows][16 B] (row XOR 4 * k-group: the four lanes that stage one
// row write four different bank groups, the fragment reads stay consecutive) + B [term][k-group][BN columns][16 B] = 32 KB; two stages
// (64 KB: two workgroups per CU).  Tile kt + 1 travels global -> registers while tile kt is multiplied, is split and stored to the other
// stage afterwards; one barrier per K-step.  The gather is plain C++ (float4 loads, 16-byte LDS stores); the waits are the compiler's.
// Epilogue in the accumulator layout: back to the operands' scale, + bias, activation, + residual, store (a wave stores 128-byte row
// segments), the bound of the stored values into y_amax.  Every output element is written exactly once: no split-K, no atomics on y.
//
// The stride-2 downsampling convolutions (block1, block{i}_conv: zero padding 1, x [F][H][W][C_in] -> y [F][Ho][Wo][C_out],
// npvp_conv3x3s2_*) are the same kernel with STRIDE = 2: only which pixel a tile row is and where its taps lie differ.  C_in % 32 == 0
// there (block1 of the ngf = 32 encoders): a K-step of 32 still lies inside one tap, one K-step per tap at C_in = 32.
//
// The decoder's transposed convolutions (ConvTranspose2d stride 2, padding 1, output_padding 1: x [F][H][W][C_in] -> y [F][2H][2W][C_out],
// npvp_convt3x3s2_*) are a third form, UP: the output splits into four pixel classes by parity, a workgroup belongs to one class, a tile
// row is an INPUT-grid position and the K loop walks the class's 1, 2 or 4 taps (9 taps per 4 outputs: no inserted zero is multiplied);
// one launch holds the four classes, the 4-tap class first.  Tiles, stages, arithmetic, barrier and the amax commit are shared source.
#include "gemm.h"
#include "f16_split.h"
#include "conv3x3_index.h"

namespace npvp {

struct Conv3x3Params {
  const float* x; const _Float16* planes; const float* bias; const float* res; float* y;
  int H, W, Cin, Cout; long long M; int pad_mode, act;      // H, W: the INPUT grid; M: output pixels
  const float* x_amax; const float* w_amax; float* y_amax;
  Conv3x3Plan plan;
};

// STRIDE 1: the "same" convolution, a tile row m is the pixel (f, h, w) of the H x W grid.  STRIDE 2 (zero padding 1, the downsampling
// convolutions): a tile row m is the OUTPUT pixel (f, oh, ow) of the Ho x Wo grid (conv3x3s2_out) and its taps are resolved by
// conv3x3s2_src inside frame f of the H x W input; p.M = F Ho Wo and p.pad_mode is not read.  Everything else is shared.
// UP (the decoder's transposed convolutions, stride 2, padding 1, output_padding 1: x [F][H][W][C_in] -> y [F][2H][2W][C_out]): a
// workgroup belongs to ONE pixel class (a, b) of the output (convt3x3s2_tile); a tile row m of M = F H W is the INPUT-grid position
// (f, i, j), stored at output pixel (f, 2 i + a, 2 j + b); the K loop walks that class's 1, 2 or 4 taps only (convt3x3s2_tap /
// convt3x3s2_src: K = taps * C_in) and reads the K-steps of those taps from the nine-tap planes.  p.plan is the plan of ONE class.
template <int TN, int STRIDE = 1, bool UP = false>
__global__ __launch_bounds__(256, 2) void conv3x3_f16_kernel(Conv3x3Params p) {
  static_assert(STRIDE == 1 || STRIDE == 2, "stride 1 or 2");
  static_assert(!UP || STRIDE == 2, "the transposed form is the stride-2 one");
  constexpr int TM = 2, WN = 2, BM = 128, BN = WN * TN * 32;
  constexpr int KGS_A = BM * 16, A_PLANE = 4 * KGS_A, A_BYTES = 2 * A_PLANE;
  constexpr int KGS_B = BN * 16, B_PLANE = 4 * KGS_B, B_BYTES = 2 * B_PLANE;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int NB = (8 * BN) / 256;                   // 16-byte pieces of a B tile per thread
  static_assert(2 * STAGE <= 65536, "two stages in 64 KB");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  int m0, m1, n0, n1, cls = 0;
  if constexpr (UP) convt3x3s2_tile(p.plan, blockIdx.x, p.M, cls, m0, m1, n0, n1);
  else conv3x3_tile(p.plan, blockIdx.x, p.M, m0, m1, n0, n1);
  const int pa = cls >> 1, pb = cls & 1, ntb = convt3x3s2_ntaps(pb);            // (UP only: the class's parities, its taps per row of taps)
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const float sa = amax_scale(amax_slot_read(p.x_amax)), sb = amax_scale(amax_slot_read(p.w_amax));
  const unsigned int cpeek = amax_peek_block(p.y_amax);
  const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout, HW = H * W;
  const int Wo = (STRIDE == 1 || UP) ? W : conv3x3s2_out(W), HWo = (STRIDE == 1 || UP) ? HW : conv3x3s2_out(H) * Wo;      // the grid the rows index
  const int spt = Cin >> 5, nk = (UP ? convt3x3s2_ntaps(pa) * ntb : 9) * spt;       // K-steps per tap; K-steps

  // A staging: thread (rl, g) stages k-group g of rows rl and rl + 64 of the tile (rows past M: the last row, computed and not stored)
  const int g = t & 3, rl = t >> 2;
  int ph[2], pw[2];
  long long fbase[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long m = (long long)m0 + rl + 64 * q < p.M ? (long long)m0 + rl + 64 * q : p.M - 1;
    const int f = (int)(m / HWo), rem = (int)(m - (long long)f * HWo);
    ph[q] = rem / Wo; pw[q] = rem - ph[q] * Wo;
    fbase[q] = (long long)f * HW;
  }
  // B staging: piece i = t + 256 j of the tile's [term][k-group][column] pieces
  const long long plane_halves = 9ll * Cin * Cout;
  long long b_src[NB];
  int b_dst[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int i = t + 256 * j, c = i % BN, slab = i / BN, s = slab >> 2, kg = slab & 3;
    b_src[j] = (long long)s * plane_halves + ((long long)kg * Cout + n0 + c) * 8;
    b_dst[j] = A_BYTES + s * B_PLANE + kg * KGS_B + c * 16;
  }
  const long long b_step = 32ll * Cout;                // halves per K-step: four k-groups of [Cout][8]

  f32x4 ra[2][2];
  f16x8 rb[NB];
  long long aoff[2] = {-1, -1};
  int kh = 0, kw = 0, cs = 0, kt_load = 0;             // the tap and the channel step of the NEXT load (loads go kt = 0, 1, 2, ...)
                                                       // (UP: kh, kw count the class's taps; kt_load is the K-step of the planes)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load = [&]() __attribute__((always_inline)) {
    if (cs == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        int sh, sw;
        if constexpr (UP) { sh = convt3x3s2_src(ph[q], pa, kh, H); sw = convt3x3s2_src(pw[q], pb, kw, W); }
        else if constexpr (STRIDE == 1) { sh = conv3x3_src(ph[q], kh, H, p.pad_mode); sw = conv3x3_src(pw[q], kw, W, p.pad_mode); }
        else { sh = conv3x3s2_src(ph[q], kh, H); sw = conv3x3s2_src(pw[q], kw, W); }
        aoff[q] = (sh < 0 || sw < 0) ? -1ll : (fbase[q] + (long long)sh * W + sw) * Cin + g * 8;
      }
      if constexpr (UP) kt_load = (convt3x3s2_tap(pa, kh) * 3 + convt3x3s2_tap(pb, kw)) * spt;         // the first K-step of this tap's kernel index
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (aoff[q] >= 0) {
        const float* src = p.x + aoff[q] + cs * 32;
        ra[q][0] = *reinterpret_cast<const f32x4*>(src);
        ra[q][1] = *reinterpret_cast<const f32x4*>(src + 4);
      } else { ra[q][0] = zero4; ra[q][1] = zero4; }
    }
    const _Float16* bsrc = p.planes + (long long)kt_load * b_step;
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = *reinterpret_cast<const f16x8*>(bsrc + b_src[j]);
    ++kt_load;
    if (++cs == spt) { cs = 0; if (++kw == (UP ? ntb : 3)) { kw = 0; ++kh; } }
  };
  auto store = [&](char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f16x4 h0, l0, h1, l1;
      split_f16_scaled(ra[q][0], sa, h0, l0);
      split_f16_scaled(ra[q][1], sa, h1, l1);
      const int off = g * KGS_A + (((rl + 64 * q) ^ (4 * g)) * 16);
      *reinterpret_cast<f16x8*>(st + off) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
      *reinterpret_cast<f16x8*>(st + A_PLANE + off) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<f16x8*>(st + b_dst[j]) = rb[j];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  auto compute = [&](const char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kg = 2 * ks + h;                       // this lane's k-group of the 16-deep sub-step
      f16x8 fa[2][TM], fb[2][TN];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[s][i] = *reinterpret_cast<const f16x8*>(st + s * A_PLANE + kg * KGS_A + (((wm * 64 + i * 32 + r) ^ (4 * kg)) * 16));
#pragma unroll
        for (int j = 0; j < TN; ++j)
          fb[s][j] = *reinterpret_cast<const f16x8*>(st + A_BYTES + s * B_PLANE + kg * KGS_B + (wn * TN * 32 + j * 32 + r) * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        /* smallest terms first, as gemm_f16_body */
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[1][i], fb[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[1][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
      }
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

  // epilogue: accumulator e of lane (r, h) of block (i, j) is row (e & 3) + 8 (e >> 2) + 4 h, column r of the 32 x 32 block
  const float ia = pow2_recip(sa), ib = pow2_recip(sb);          // (two exact scalings: neither product of scales can leave fp32's range)
  float cmax = 0.f;
  if constexpr (UP) {
    // rows outer (one division per group of four consecutive rows, then carries): row m = (f, i, j) -> output pixel (f, 2 i + a, 2 j + b)
    float bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bias[j] = p.bias[n0 + wn * TN * 32 + j * 32 + r];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int eg = 0; eg < 4; ++eg) {
        const long long mg = (long long)m0 + wm * 64 + i * 32 + 8 * eg + 4 * h;
        int f = (int)(mg / HW), rem = (int)(mg - (long long)f * HW);
        int ri = rem / W, rj = rem - ri * W;
#pragma unroll
        for (int el = 0; el < 4; ++el) {
          if (mg + el < m1) {
            const long long pix = ((long long)f * 2 * H + 2 * ri + pa) * (2 * W) + 2 * rj + pb;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const float v = ae_act(acc[i][j][4 * eg + el] * ia * ib + bias[j], p.act);
              p.y[pix * Cout + n0 + wn * TN * 32 + j * 32 + r] = v;
              cmax = fmaxf(cmax, fabsf(v));
            }
          }
          if (++rj == W) { rj = 0; if (++ri == H) { ri = 0; ++f; } }
        }
      }
  } else {
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * TN * 32 + j * 32 + r;
    const float b = p.bias[col];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const long long m = (long long)m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (m < m1) {
          float v = ae_act(acc[i][j][e] * ia * ib + b, p.act);
          if (p.res) v += p.res[m * Cout + col];
          p.y[m * Cout + col] = v;
          cmax = fmaxf(cmax, fabsf(v));
        }
      }
  }
  }
  amax_slot_commit_block(p.y_amax, cmax, reinterpret_cast<float*>(lds), cpeek);       // (the stages are idle after the loop's last barrier)
}

// w [Cout][Cin][3][3] -> planes [term][9 Cin / 8][Cout][8 over k], k = (kh * 3 + kw) * Cin + ci: split_weights_f16_kernel's arithmetic on
// the gathered matrix [Cout][9 Cin].  wt != 0: w is a ConvTranspose2d weight [Cin][Cout][3][3]; the same planes, the kernel index unflipped.
__global__ __launch_bounds__(256) void conv3x3_planes_kernel(const float* __restrict__ w, int Cin, int Cout, _Float16* __restrict__ out,
                                                             const float* __restrict__ amax, int wt) {
  const long long slots = 9ll * Cin * Cout / 8, plane = 9ll * Cin * Cout;
  const float s = amax_scale(amax_slot_read(amax));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i % Cout), kb = (int)(i / Cout), k0 = kb * 8, tap = k0 / Cin, ci = k0 - tap * Cin;
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = w[(wt ? (long long)(ci + e) * Cout + n : (long long)n * Cin + ci + e) * 9 + tap] * s;
      hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]);
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = hi;
    *reinterpret_cast<f16x8*>(out + plane + i * 8) = lo;
  }
}

__global__ __launch_bounds__(256) void conv3x3_zero_slot_kernel(float* slot) {
  for (int i = threadIdx.x; i < AMAX_WORDS * AMAX_STRIDE; i += 256) slot[i] = 0.f;
}

}  // namespace npvp

using namespace npvp;

static bool conv3x3_shape_ok(int F, int H, int W, int C_in, int C_out) {
  return F > 0 && H > 0 && W > 0 && C_in > 0 && C_out > 0 && C_in % 64 == 0 && C_out % 64 == 0 && (long long)F * H * W < (1ll << 31) &&
         9ll * C_in < (1ll << 31);
}

extern "C" long long npvp_conv3x3_planes_bytes(int C_in, int C_out) {
  if (C_in <= 0 || C_out <= 0 || C_in % 64 || C_out % 64) return -1;
  return 2ll * 9 * C_in * C_out * 2;
}

// the stride-2 entry points' channel rule: a K-step of 32 inside one tap, 64-column tiles
static bool conv3x3s2_channels_ok(int C_in, int C_out) { return C_in > 0 && C_out > 0 && C_in % 32 == 0 && C_out % 64 == 0; }

static bool conv3x3s2_shape_ok(int F, int H, int W, int C_in, int C_out) {
  return F > 0 && H > 0 && W > 0 && conv3x3s2_channels_ok(C_in, C_out) && (long long)H * W < (1ll << 31) &&
         (long long)F * conv3x3s2_out(H) * conv3x3s2_out(W) < (1ll << 31) && 9ll * C_in < (1ll << 31);
}

#define CONV3X3S2_SHAPE_MSG "conv3x3s2: F, H, W >= 1, C_in a multiple of 32, C_out a multiple of 64, H * W and F * Ho * Wo below 2^31"

extern "C" long long npvp_conv3x3s2_planes_bytes(int C_in, int C_out) {
  if (!conv3x3s2_channels_ok(C_in, C_out)) return -1;
  return 2ll * 9 * C_in * C_out * 2;
}

// zero the slot, the weight's amax into it, the scaled two-term planes (conv3x3_planes_kernel itself needs C_in % 8 == 0 only)
// (wt != 0: w is a ConvTranspose2d weight [C_in][C_out][3][3])
static int conv3x3_planes_launch(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream, int wt = 0);

extern "C" int npvp_conv3x3s2_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "conv3x3s2_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(conv3x3s2_channels_ok(C_in, C_out), "conv3x3s2_planes: C_in must be a multiple of 32 and C_out a multiple of 64");
  NPVP_CHECK_ARG(((uintptr_t)w % 16) == 0 && ((uintptr_t)planes % 16) == 0, "conv3x3s2_planes: w and planes must be 16-byte aligned");
  return conv3x3_planes_launch(w, C_in, C_out, planes, w_amax, stream);
}

extern "C" int npvp_conv3x3_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "conv3x3_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(C_in > 0 && C_out > 0 && C_in % 64 == 0 && C_out % 64 == 0, "conv3x3_planes: C_in and C_out must be multiples of 64");
  NPVP_CHECK_ARG(((uintptr_t)w % 16) == 0 && ((uintptr_t)planes % 16) == 0, "conv3x3_planes: w and planes must be 16-byte aligned");
  return conv3x3_planes_launch(w, C_in, C_out, planes, w_amax, stream);
}

static int conv3x3_planes_launch(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream, int wt) {
  NPVP_LAUNCH(conv3x3_zero_slot_kernel, dim3(1), dim3(256), 0, stream, w_amax);          // (a kernel, not a memset node: see gemm_f16.hip)
  NPVP_CHECK_LAUNCH();
  const int rc = wt ? npvp_amax(w, C_in, 9ll * C_out, 9ll * C_out, w_amax, stream) : npvp_amax(w, C_out, 9ll * C_in, 9ll * C_in, w_amax, stream);
  if (rc != NPVP_OK) return rc;
  const long long slots = 9ll * C_in * C_out / 8;
  long long blocks = (slots + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  NPVP_LAUNCH(conv3x3_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, w, C_in, C_out, (_Float16*)planes, (const float*)w_amax, wt);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_conv3x3_route(int F, int H, int W, int C_in, int C_out, int* out6) {
  NPVP_CHECK_ARG(out6 && conv3x3_shape_ok(F, H, W, C_in, C_out),
                 "conv3x3: F, H, W >= 1, C_in and C_out multiples of 64, F * H * W below 2^31");
  const Conv3x3Plan p = conv3x3_plan((long long)F * H * W, C_out);
  out6[0] = p.variant; out6[1] = p.bm; out6[2] = p.bn; out6[3] = p.tiles_m; out6[4] = p.tiles_n; out6[5] = p.grid;
  return NPVP_OK;
}

extern "C" int npvp_conv3x3_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4) {
  NPVP_CHECK_ARG(out4 && conv3x3_shape_ok(F, H, W, C_in, C_out),
                 "conv3x3: F, H, W >= 1, C_in and C_out multiples of 64, F * H * W below 2^31");
  const long long M = (long long)F * H * W;
  const Conv3x3Plan p = conv3x3_plan(M, C_out);
  NPVP_CHECK_ARG(block >= 0 && block < p.grid, "conv3x3_tile: block outside the plan's grid");
  conv3x3_tile(p, block, M, out4[0], out4[1], out4[2], out4[3]);
  return NPVP_OK;
}

extern "C" int npvp_conv3x3_src(int c, int tap, int extent, int pad_mode) {
  if (tap < 0 || tap > 2 || (pad_mode != 0 && pad_mode != 1) || extent < 1 + pad_mode || c < 0 || c >= extent) return -2;
  return conv3x3_src(c, tap, extent, pad_mode);
}

extern "C" int npvp_conv3x3_f16(const float* x, const void* planes, const float* bias, const float* residual, float* y, int F, int H,
                                int W, int C_in, int C_out, int pad_mode, int act, const float* x_amax, const float* w_amax,
                                float* y_amax, void* workspace, long long ws_bytes, hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(x && planes && bias && y && x_amax && w_amax, "conv3x3: x, planes, bias, y, x_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(conv3x3_shape_ok(F, H, W, C_in, C_out), "conv3x3: F, H, W >= 1, C_in and C_out multiples of 64, F * H * W below 2^31");
  NPVP_CHECK_ARG(pad_mode == 0 || pad_mode == 1, "conv3x3: pad_mode 0 (zero) or 1 (reflect)");
  NPVP_CHECK_ARG(pad_mode == 0 || (H >= 2 && W >= 2), "conv3x3: reflection padding needs H, W >= 2");
  NPVP_CHECK_ARG(act >= 0 && act <= 3, "conv3x3: act in 0..3");
  NPVP_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)planes % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)residual % 16) == 0,
                 "conv3x3: x, planes, y and residual must be 16-byte aligned");
  Conv3x3Params p;
  p.x = x; p.planes = (const _Float16*)planes; p.bias = bias; p.res = residual; p.y = y;
  p.H = H; p.W = W; p.Cin = C_in; p.Cout = C_out; p.M = (long long)F * H * W; p.pad_mode = pad_mode; p.act = act;
  p.x_amax = x_amax; p.w_amax = w_amax; p.y_amax = y_amax;
  p.plan = conv3x3_plan(p.M, C_out);
  if (p.plan.variant == 1) NPVP_LAUNCH((conv3x3_f16_kernel<2>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  else NPVP_LAUNCH((conv3x3_f16_kernel<1>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// ---- stride 2, zero padding 1
extern "C" int npvp_conv3x3s2_route(int F, int H, int W, int C_in, int C_out, int* out8) {
  NPVP_CHECK_ARG(out8 && conv3x3s2_shape_ok(F, H, W, C_in, C_out), CONV3X3S2_SHAPE_MSG);
  const int Ho = conv3x3s2_out(H), Wo = conv3x3s2_out(W);
  const Conv3x3Plan p = conv3x3_plan((long long)F * Ho * Wo, C_out);
  out8[0] = p.variant; out8[1] = p.bm; out8[2] = p.bn; out8[3] = p.tiles_m; out8[4] = p.tiles_n; out8[5] = p.grid;
  out8[6] = Ho; out8[7] = Wo;
  return NPVP_OK;
}

extern "C" int npvp_conv3x3s2_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4) {
  NPVP_CHECK_ARG(out4 && conv3x3s2_shape_ok(F, H, W, C_in, C_out), CONV3X3S2_SHAPE_MSG);
  const long long M = (long long)F * conv3x3s2_out(H) * conv3x3s2_out(W);
  const Conv3x3Plan p = conv3x3_plan(M, C_out);
  NPVP_CHECK_ARG(block >= 0 && block < p.grid, "conv3x3s2_tile: block outside the plan's grid");
  conv3x3_tile(p, block, M, out4[0], out4[1], out4[2], out4[3]);
  return NPVP_OK;
}

extern "C" int npvp_conv3x3s2_src(int o, int tap, int extent) {
  if (tap < 0 || tap > 2 || extent < 1 || o < 0 || o >= conv3x3s2_out(extent)) return -2;
  return conv3x3s2_src(o, tap, extent);
}

extern "C" int npvp_conv3x3s2_f16(const float* x, const void* planes, const float* bias, const float* residual, float* y, int F, int H,
                                  int W, int C_in, int C_out, int act, const float* x_amax, const float* w_amax, float* y_amax,
                                  void* workspace, long long ws_bytes, hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(x && planes && bias && y && x_amax && w_amax, "conv3x3s2: x, planes, bias, y, x_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(conv3x3s2_shape_ok(F, H, W, C_in, C_out), CONV3X3S2_SHAPE_MSG);
  NPVP_CHECK_ARG(act >= 0 && act <= 3, "conv3x3s2: act in 0..3");
  NPVP_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)planes % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)residual % 16) == 0,
                 "conv3x3s2: x, planes, y and residual must be 16-byte aligned");
  Conv3x3Params p;
  p.x = x; p.planes = (const _Float16*)planes; p.bias = bias; p.res = residual; p.y = y;
  p.H = H; p.W = W; p.Cin = C_in; p.Cout = C_out; p.M = (long long)F * conv3x3s2_out(H) * conv3x3s2_out(W); p.pad_mode = 0; p.act = act;
  p.x_amax = x_amax; p.w_amax = w_amax; p.y_amax = y_amax;
  p.plan = conv3x3_plan(p.M, C_out);
  if (p.plan.variant == 1) NPVP_LAUNCH((conv3x3_f16_kernel<2, 2>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  else NPVP_LAUNCH((conv3x3_f16_kernel<1, 2>), dim3((unsigned)p.plan.grid), dim3(256), 0, stream, p);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

// ---- transposed, stride 2, padding 1, output_padding 1 (the decoder's upsampling convolutions)
static bool convt3x3s2_shape_ok(int F, int H, int W, int C_in, int C_out) {
  return F > 0 && H > 0 && W > 0 && conv3x3s2_channels_ok(C_in, C_out) && 4ll * F * H * W < (1ll << 31) && 9ll * C_in < (1ll << 31);
}

#define CONVT3X3S2_SHAPE_MSG "convt3x3s2: F, H, W >= 1, C_in a multiple of 32, C_out a multiple of 64, F * 2H * 2W below 2^31"

extern "C" int npvp_convt3x3s2_ntaps(int parity) { return parity == 0 || parity == 1 ? convt3x3s2_ntaps(parity) : -2; }

extern "C" int npvp_convt3x3s2_tap(int parity, int t) {
  if ((parity != 0 && parity != 1) || t < 0 || t >= convt3x3s2_ntaps(parity)) return -2;
  return convt3x3s2_tap(parity, t);
}

extern "C" int npvp_convt3x3s2_src(int i, int parity, int t, int extent) {
  if ((parity != 0 && parity != 1) || t < 0 || t >= convt3x3s2_ntaps(parity) || extent < 1 || i < 0 || i >= extent) return -2;
  return convt3x3s2_src(i, parity, t, extent);
}

extern "C" long long npvp_convt3x3s2_planes_bytes(int C_in, int C_out) {
  if (!conv3x3s2_channels_ok(C_in, C_out)) return -1;
  return 2ll * 9 * C_in * C_out * 2;
}

extern "C" int npvp_convt3x3s2_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, hipStream_t stream) {
  NPVP_CHECK_ARG(w && planes && w_amax, "convt3x3s2_planes: w, planes and w_amax must be non-null");
  NPVP_CHECK_ARG(conv3x3s2_channels_ok(C_in, C_out), "convt3x3s2_planes: C_in must be a multiple of 32 and C_out a multiple of 64");
  NPVP_CHECK_ARG(((uintptr_t)w % 16) == 0 && ((uintptr_t)planes % 16) == 0, "convt3x3s2_planes: w and planes must be 16-byte aligned");
  return conv3x3_planes_launch(w, C_in, C_out, planes, w_amax, stream, 1);
}

extern "C" int npvp_convt3x3s2_route(int F, int H, int W, int C_in, int C_out, int* out8) {
  NPVP_CHECK_ARG(out8 && convt3x3s2_shape_ok(F, H, W, C_in, C_out), CONVT3X3S2_SHAPE_MSG);
  const Conv3x3Plan p = conv3x3_plan((long long)F * H * W, C_out);
  out8[0] = p.variant; out8[1] = p.bm; out8[2] = p.bn; out8[3] = p.tiles_m; out8[4] = p.tiles_n; out8[5] = convt3x3s2_grid(p);
  out8[6] = 2 * H; out8[7] = 2 * W;
  return NPVP_OK;
}

extern "C" int npvp_convt3x3s2_tile(int F, int H, int W, int C_in, int C_out, int block, int* out6) {
  NPVP_CHECK_ARG(out6 && convt3x3s2_shape_ok(F, H, W, C_in, C_out), CONVT3X3S2_SHAPE_MSG);
  const long long M = (long long)F * H * W;
  const Conv3x3Plan p = conv3x3_plan(M, C_out);
  NPVP_CHECK_ARG(block >= 0 && block < convt3x3s2_grid(p), "convt3x3s2_tile: block outside the plan's grid");
  int cls;
  convt3x3s2_tile(p, block, M, cls, out6[2], out6[3], out6[4], out6[5]);
  out6[0] = cls >> 1; out6[1] = cls & 1;
  return NPVP_OK;
}

extern "C" int npvp_convt3x3s2_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in,
                                   int C_out, int act, const float* x_amax, const float* w_amax, float* y_amax, void* workspace,
                                   long long ws_bytes, hipStream_t stream) {
  (void)workspace; (void)ws_bytes;
  NPVP_CHECK_ARG(x && planes && bias && y && x_amax && w_amax, "convt3x3s2: x, planes, bias, y, x_amax and w_amax must be non-null");
  NPVP_CHECK_ARG(convt3x3s2_shape_ok(F, H, W, C_in, C_out), CONVT3X3S2_SHAPE_MSG);
  NPVP_CHECK_ARG(act >= 0 && act <= 3, "convt3x3s2: act in 0..3");
  NPVP_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)planes % 16) == 0 && ((uintptr_t)y % 16) == 0,
                 "convt3x3s2: x, planes and y must be 16-byte aligned");
  Conv3x3Params p;
  p.x = x; p.planes = (const _Float16*)planes; p.bias = bias; p.res = nullptr; p.y = y;
  p.H = H; p.W = W; p.Cin = C_in; p.Cout = C_out; p.M = (long long)F * H * W; p.pad_mode = 0; p.act = act;
  p.x_amax = x_amax; p.w_amax = w_amax; p.y_amax = y_amax;
  p.plan = conv3x3_plan(p.M, C_out);                     // the tiles of ONE pixel class; the launch holds four of them
  const unsigned grid = (unsigned)convt3x3s2_grid(p.plan);
  if (p.plan.variant == 1) NPVP_LAUNCH((conv3x3_f16_kernel<2, 2, true>), dim3(grid), dim3(256), 0, stream, p);
  else NPVP_LAUNCH((conv3x3_f16_kernel<1, 2, true>), dim3(grid), dim3(256), 0, stream, p);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
