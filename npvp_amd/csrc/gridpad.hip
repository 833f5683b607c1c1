// Centre padding of a feature grid to the next multiple of the attention window, and its adjoint
// (ref/models/VidHRFormer.py:488-511, PadBlock.pad_if_needed / depad_if_needed), on token rows [frames][H*W][C]:
//   pad: src [F*H*W, C]    -> dst [rows_out >= F*Hp*Wp, C]: a copy of the source row or zeros, EVERY element written once
//   cut: src [>= F*Hp*Wp, C] -> dst [F*H*W, C] = the centre rows (+ an addend)
// Both are HBM-bound copies: 16-byte accesses, a capped grid with a grid-stride loop over rows, the row -> (frame, h, w) decode once
// per row with multiply-shift divisions (div_magic), two rows in flight per thread.  No atomics but the amax word: bit-reproducible.
#include "common.h"

namespace npvp {

struct GridPadGeom {
  int H, W, Hp, Wp, top, left;
  unsigned int inner, outer;                // H*W, Hp*Wp
  unsigned int m_frame, m_line;             // magic of the iteration space: rows per frame, rows per grid line
  int s_frame, s_line;
};

// dst row r of the padded layout -> its source row, or -1 (border, or a trailing row past F*Hp*Wp)
__device__ __forceinline__ long long pad_source_row(const GridPadGeom& g, unsigned int r, unsigned int body) {
  if (r >= body) return -1;
  const unsigned int f = div_by_magic(r, g.m_frame, g.s_frame);
  const unsigned int rem = r - f * g.outer;
  const unsigned int hp = div_by_magic(rem, g.m_line, g.s_line);
  const int h = (int)hp - g.top, w = (int)(rem - hp * (unsigned int)g.Wp) - g.left;
  if ((unsigned int)h >= (unsigned int)g.H || (unsigned int)w >= (unsigned int)g.W) return -1;
  return (long long)f * g.inner + (long long)h * g.W + w;
}

// dst row r of the cut layout -> its source row in the padded layout
__device__ __forceinline__ long long cut_source_row(const GridPadGeom& g, unsigned int r) {
  const unsigned int f = div_by_magic(r, g.m_frame, g.s_frame);
  const unsigned int rem = r - f * g.inner;
  const unsigned int h = div_by_magic(rem, g.m_line, g.s_line);
  const unsigned int w = rem - h * (unsigned int)g.W;
  return (long long)f * g.outer + (long long)(h + g.top) * g.Wp + (w + g.left);
}

// 256 threads = (256 >> lg) rows x (1 << lg) lanes of float4; lanes stride over the row when C/4 > lanes
__global__ __launch_bounds__(256) void grid_center_pad_kernel(const float* __restrict__ src, long long ld_src, float* __restrict__ dst,
                                                              long long ld_dst, GridPadGeom g, unsigned int body, unsigned int rows_out,
                                                              int c4n, int lg, float* __restrict__ amax) {
  __shared__ float ared[4];
  const unsigned int peek = amax_peek_block(amax);
  const int lanes = 1 << lg, lane = threadIdx.x & (lanes - 1);
  const unsigned int rpb = 256u >> lg, step = gridDim.x * rpb;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float am = 0.f;
  // (rows_out < 2^31 and step <= 2^19: r + step does not wrap)
  for (unsigned int r = blockIdx.x * rpb + (threadIdx.x >> lg); r < rows_out; r += 2 * step) {
    const unsigned int r2 = r + step;
    const long long s1 = pad_source_row(g, r, body);
    const long long s2 = r2 < rows_out ? pad_source_row(g, r2, body) : -1;
    for (int c = lane; c < c4n; c += lanes) {
      const float4 v1 = s1 >= 0 ? ld4(src + s1 * ld_src + 4 * c) : zero;
      const float4 v2 = s2 >= 0 ? ld4(src + s2 * ld_src + 4 * c) : zero;
      st4(dst + (long long)r * ld_dst + 4 * c, v1);
      if (r2 < rows_out) st4(dst + (long long)r2 * ld_dst + 4 * c, v2);
      am = amax4(amax4(am, v1), v2);
    }
  }
  amax_slot_commit_block(amax, am, ared, peek);
}

__global__ __launch_bounds__(256) void grid_center_cut_kernel(const float* __restrict__ src, long long ld_src,
                                                              const float* __restrict__ addend, long long ld_add, float* __restrict__ dst,
                                                              long long ld_dst, GridPadGeom g, unsigned int rows, int c4n, int lg,
                                                              float* __restrict__ amax) {
  __shared__ float ared[4];
  const unsigned int peek = amax_peek_block(amax);
  const int lanes = 1 << lg, lane = threadIdx.x & (lanes - 1);
  const unsigned int rpb = 256u >> lg, step = gridDim.x * rpb;
  float am = 0.f;
  for (unsigned int r = blockIdx.x * rpb + (threadIdx.x >> lg); r < rows; r += 2 * step) {
    const unsigned int r2 = r + step;
    const bool two = r2 < rows;
    const long long s1 = cut_source_row(g, r);
    const long long s2 = two ? cut_source_row(g, r2) : s1;
    for (int c = lane; c < c4n; c += lanes) {
      float4 v1 = ld4(src + s1 * ld_src + 4 * c);
      float4 v2 = ld4(src + s2 * ld_src + 4 * c);
      if (addend) {
        const float4 a1 = ld4(addend + (long long)r * ld_add + 4 * c);
        const float4 a2 = ld4(addend + (long long)(two ? r2 : r) * ld_add + 4 * c);
        v1.x += a1.x; v1.y += a1.y; v1.z += a1.z; v1.w += a1.w;
        v2.x += a2.x; v2.y += a2.y; v2.z += a2.z; v2.w += a2.w;
      }
      st4(dst + (long long)r * ld_dst + 4 * c, v1);
      if (two) st4(dst + (long long)r2 * ld_dst + 4 * c, v2);
      am = amax4(amax4(am, v1), v2);          // (without a second row v2 repeats v1: the bound is unchanged)
    }
  }
  amax_slot_commit_block(amax, am, ared, peek);
}

// lanes per row: the smallest power of two >= C/4, at most 256
static inline int gridpad_lane_bits(int c4n) {
  int lg = 0;
  while (lg < 8 && (1 << lg) < c4n) ++lg;
  return lg;
}

static inline int gridpad_blocks(long long rows, int lg) {
  const long long rpb = 256 >> lg;
  long long b = (rows + rpb - 1) / rpb;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace npvp

using namespace npvp;

static int gridpad_check(const char*& why, int F, int H, int W, int Hp, int Wp, int top, int left, int C, long long ld_a, long long ld_b) {
  why = nullptr;
  if (F < 0 || H <= 0 || W <= 0 || C <= 0) why = "grid pad: bad shape";
  else if (Hp < H || Wp < W) why = "grid pad: the padded grid is smaller than the grid";
  else if (top < 0 || top > Hp - H || left < 0 || left > Wp - W) why = "grid pad: the grid does not lie inside the padded grid";
  else if (C % 4 != 0) why = "grid pad: C must be a multiple of 4";
  else if (ld_a % 4 != 0 || ld_b % 4 != 0 || ld_a < C || ld_b < C) why = "grid pad: row strides must be multiples of 4 and at least C";
  else if ((long long)(F > 0 ? F : 1) * Hp * Wp >= (1ll << 31)) why = "grid pad: row counts must fit 32 bits";
  return why ? NPVP_ERR_ARG : NPVP_OK;
}

static GridPadGeom gridpad_geom(int H, int W, int Hp, int Wp, int top, int left, bool padded_space) {
  GridPadGeom g;
  g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp; g.top = top; g.left = left;
  g.inner = (unsigned int)(H * W); g.outer = (unsigned int)(Hp * Wp);
  div_magic(padded_space ? g.outer : g.inner, g.m_frame, g.s_frame);
  div_magic((unsigned int)(padded_space ? Wp : W), g.m_line, g.s_line);
  return g;
}

extern "C" int npvp_grid_center_pad(const float* src, long long ld_src, float* dst, long long ld_dst, int F, int H, int W, int Hp, int Wp,
                                    int top, int left, int C, long long rows_out, float* dst_amax, hipStream_t stream) {
  const char* why;
  if (gridpad_check(why, F, H, W, Hp, Wp, top, left, C, ld_src, ld_dst) != NPVP_OK) NPVP_CHECK_ARG(false, why);
  const long long body = (long long)F * Hp * Wp;
  NPVP_CHECK_ARG(rows_out >= body && rows_out > 0 && rows_out < (1ll << 31), "grid pad: rows_out must cover F*Hp*Wp and fit 32 bits");
  NPVP_CHECK_ARG(dst && (src || F == 0), "grid pad: null buffer");
  NPVP_CHECK_ARG(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "grid pad: buffers must be 16-byte aligned");
  const int c4n = C / 4, lg = gridpad_lane_bits(c4n);
  const GridPadGeom g = gridpad_geom(H, W, Hp, Wp, top, left, true);
  NPVP_LAUNCH(grid_center_pad_kernel, dim3(gridpad_blocks(rows_out, lg)), dim3(256), 0, stream, src, ld_src, dst, ld_dst, g,
              (unsigned int)body, (unsigned int)rows_out, c4n, lg, dst_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}

extern "C" int npvp_grid_center_cut(const float* src, long long ld_src, const float* addend, long long ld_add, float* dst, long long ld_dst,
                                    int F, int H, int W, int Hp, int Wp, int top, int left, int C, float* dst_amax, hipStream_t stream) {
  const char* why;
  if (gridpad_check(why, F, H, W, Hp, Wp, top, left, C, ld_src, ld_dst) != NPVP_OK) NPVP_CHECK_ARG(false, why);
  NPVP_CHECK_ARG(F > 0 && src && dst, "grid cut: empty shape or null buffer");
  NPVP_CHECK_ARG(!addend || (ld_add % 4 == 0 && ld_add >= C), "grid cut: the addend's row stride must be a multiple of 4 and at least C");
  NPVP_CHECK_ARG(((uintptr_t)src | (uintptr_t)dst | (uintptr_t)addend) % 16 == 0, "grid cut: buffers must be 16-byte aligned");
  const long long rows = (long long)F * H * W;
  const int c4n = C / 4, lg = gridpad_lane_bits(c4n);
  const GridPadGeom g = gridpad_geom(H, W, Hp, Wp, top, left, false);
  NPVP_LAUNCH(grid_center_cut_kernel, dim3(gridpad_blocks(rows, lg)), dim3(256), 0, stream, src, ld_src, addend, ld_add, dst, ld_dst, g,
              (unsigned int)rows, c4n, lg, dst_amax);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
