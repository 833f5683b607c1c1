// Index math of the frozen decoder's 7 x 7 tail (conv7x7.hip: ReflectionPad2d(3) -> Conv2d(C_in, C_out <= 4, 7) -> activation) and of
// the frozen encoder's 7 x 7 stem (the same file: ReflectionPad2d(3) -> Conv2d(C_in <= 4, C_out, 7) -> activation), as
// __host__ __device__ functions: the kernels and the launchers call them, and the C ABI exports them unchanged (npvp_tail7x7_src,
// npvp_tail7x7_adj_src, npvp_tail7x7_route, npvp_tail7x7_tile, npvp_tail7x7_dgrad_route, npvp_tail7x7_dgrad_tile, npvp_stem7x7_k,
// npvp_stem7x7_route, npvp_stem7x7_tile), so which pixel a tap reads, which outputs a workgroup owns and which Z columns it holds are
// tested on the host.
#pragma once

#include "conv3x3_index.h"

namespace npvp {

// Source coordinate of tap `tap` (0..6: offsets -3..+3) at output coordinate c of an axis of `extent` >= 4 pixels behind
// ReflectionPad2d(3): -1 -> 1, -2 -> 2, -3 -> 3, extent -> extent - 2, ...  Always inside the axis: there is no zero tap.
NPVP_HD int tail7x7_src(int c, int tap, int extent) {
  const int s = c + tap - 3;
  if (s < 0) return -s;
  return s < extent ? s : 2 * extent - 2 - s;
}

// The adjoint of tail7x7_src: the OUTPUT coordinates o of the axis with tail7x7_src(o, tap, extent) == s.  There are at most two:
//   which 0, the straight one: o = s + 3 - tap, when it lies inside the axis;
//   which 1, the mirror image: o = 3 - tap - s (reflected at the low edge: tap <= 2, s >= 1) or o = 2 extent + 1 - s - tap (reflected
//            at the high edge: tap >= 4, s <= extent - 2), when it lies inside the axis.  tap 3 has no mirror.
// Returns the coordinate, or -1 when there is none.  The two are never equal (they differ by 2 s or by 2 (extent - 1 - s)).
NPVP_HD int tail7x7_adj_src(int s, int tap, int extent, int which) {
  int o;
  if (which == 0) o = s + 3 - tap;
  else if (tap <= 2) o = s >= 1 ? 3 - tap - s : -1;
  else if (tap >= 4) o = s <= extent - 2 ? 2 * extent + 1 - s - tap : -1;
  else o = -1;
  return o >= 0 && o < extent ? o : -1;
}

// The forward plan.  The kernel computes Z[(image row, column w')][(kw, co)] = sum_{kh, ci} x[row's frame, refl(h + kh - 3), w', ci] w[co, ci, kh, kw]
// for a tile of at most 128 (image row, column) pairs and sums y[row, w] = sum_kw Z[(row, refl(w + kw - 3))][(kw, co)] inside the
// workgroup, so a tile holds whole Z windows:
//   W <= 128: a tile is `rows` = 128 / W consecutive image rows of the F * H rows (frames follow each other: a tile may span frames,
//             every row gathers its kh taps inside its own frame), all W columns; the Z window is [0, W).
//   W >  128: a tile is ONE image row and a segment of `seg_cols` = 122 output columns [w0, w1); its Z window [z0, z1) is the segment
//             plus 3 halo columns per side, cut at the image edges (a reflected column lies inside the cut window): at most 128 rows.
//             The halo columns are computed by both neighbours.
struct Tail7x7Plan { int rows, segs, seg_cols, tiles_r, grid; };

NPVP_HD Tail7x7Plan tail7x7_plan(long long FH, int W) {
  Tail7x7Plan p;
  if (W <= 128) { p.rows = 128 / W; p.segs = 1; p.seg_cols = W; }
  else { p.rows = 1; p.seg_cols = 122; p.segs = (W + 121) / 122; }
  p.tiles_r = (int)((FH + p.rows - 1) / p.rows);
  p.grid = p.tiles_r * p.segs;
  return p;
}

// image rows [r0, r1) of the F * H rows, output columns [w0, w1) and Z window [z0, z1) of workgroup `block`
NPVP_HD void tail7x7_tile(const Tail7x7Plan& p, int block, long long FH, int W, int& r0, int& r1, int& w0, int& w1, int& z0, int& z1) {
  const int tr = block / p.segs, sg = block - tr * p.segs;
  r0 = tr * p.rows;
  r1 = (long long)r0 + p.rows < FH ? r0 + p.rows : (int)FH;
  w0 = sg * p.seg_cols;
  w1 = w0 + p.seg_cols < W ? w0 + p.seg_cols : W;
  z0 = w0 - 3 > 0 ? w0 - 3 : 0;
  z1 = w1 + 3 < W ? w1 + 3 : W;
}

// The input gradient's plan: conv3x3_plan's row tiles over M = F H W input pixels, 64 columns of C_in per tile (variant 1,
// C_in % 64 == 0) or 32 (variant 2); block b -> tile (b / tiles_n, b % tiles_n), rows and columns by conv3x3_tile.
NPVP_HD Conv3x3Plan tail7x7_dgrad_plan(long long M, int C_in) {
  Conv3x3Plan p;
  p.variant = C_in % 64 == 0 ? 1 : 2;
  p.bm = 128;
  p.bn = p.variant == 1 ? 64 : 32;
  p.tiles_m = (int)((M + p.bm - 1) / p.bm);
  p.tiles_n = C_in / p.bn;
  p.grid = p.tiles_m * p.tiles_n;
  return p;
}

// ---- The encoder's stem: C[M = F H W][N = C_out] = A[M][K] B[K][N] with the dense K order k = (kh * 7 + kw) * C_in + ci, zero-padded
// from 49 C_in to a multiple of 32 (C_in = 1, 2, 3, 4: 64, 128, 160, 224 - 2, 4, 5, 7 K-steps).  The tiles are tail7x7_dgrad_plan's over
// (M, C_out): 128 rows x 64 columns (C_out % 64 == 0) or x 32, rows and columns by conv3x3_tile.
NPVP_HD int stem7x7_kpad(int C_in) { return (49 * C_in + 31) / 32 * 32; }

// K index k (0 <= k < stem7x7_kpad(C_in)) -> kernel row kh, kernel column kw, input channel ci; false for an index of the zero padding
// (kh comes out as 7 or more there).  The gather of stem7x7_f16_kernel and stem7x7_planes_kernel both call it.
NPVP_HD bool stem7x7_k(int C_in, int k, int& kh, int& kw, int& ci) {
  const int tap = k / C_in;
  ci = k - tap * C_in;
  kh = tap / 7;
  kw = tap - kh * 7;
  return tap < 49;
}

}  // namespace npvp
