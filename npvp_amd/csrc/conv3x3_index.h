// Index math of the 3 x 3 implicit-GEMM convolution (conv3x3.hip), as __host__ __device__ functions: the kernel and the launcher call
// them, and the C ABI exports them unchanged (npvp_conv3x3_src, npvp_conv3x3_route, npvp_conv3x3_tile, npvp_conv3x3s2_*, npvp_convt3x3s2_*), so the part of the kernel that
// can go wrong silently - which pixel a tap reads, which outputs a workgroup owns - is tested on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NPVP_HD __host__ __device__ __forceinline__
#else
#define NPVP_HD inline
#endif

namespace npvp {

// Source coordinate of tap `tap` (0, 1, 2: offsets -1, 0, +1) at output coordinate c of an axis of `extent` pixels.
//   pad_mode 0 (zero padding): -1 outside the axis - the tap contributes 0.
//   pad_mode 1 (ReflectionPad2d(1)): -1 -> 1, extent -> extent - 2 (extent >= 2).
NPVP_HD int conv3x3_src(int c, int tap, int extent, int pad_mode) {
  const int s = c + tap - 1;
  if (s >= 0 && s < extent) return s;
  if (pad_mode == 0) return -1;
  return s < 0 ? -s : 2 * extent - 2 - s;
}

// Stride 2, zero padding 1 (the downsampling convolutions).  Outputs of an axis of `extent` pixels: floor((extent + 2 - 3) / 2) + 1.
NPVP_HD int conv3x3s2_out(int extent) { return (extent + 1) / 2; }

// Source coordinate of tap `tap` at OUTPUT coordinate o of that axis: 2 o + tap - 1, or -1 (the tap contributes 0) outside the axis -
// tap 0 of the first output, and on an odd extent tap 2 of the last output as well.
NPVP_HD int conv3x3s2_src(int o, int tap, int extent) {
  const int s = 2 * o + tap - 1;
  return s >= 0 && s < extent ? s : -1;
}

// The plan of a launch: output tiles of bm rows (output pixels, M = F H W of them, F Ho Wo at stride 2) x bn columns (output channels),
// one workgroup per tile, block b -> tile (b / tiles_n, b % tiles_n): the tiles of one row block are neighbours in launch order and share their A rows in L2.
//   variant 1: 128 x 128 tiles (C_out % 128 == 0), variant 2: 128 x 64 tiles (C_out % 64 == 0 only); 256 threads either way.
struct Conv3x3Plan { int variant, bm, bn, tiles_m, tiles_n, grid; };

NPVP_HD Conv3x3Plan conv3x3_plan(long long M, int C_out) {
  Conv3x3Plan p;
  p.variant = C_out % 128 == 0 ? 1 : 2;
  p.bm = 128;
  p.bn = p.variant == 1 ? 128 : 64;
  p.tiles_m = (int)((M + p.bm - 1) / p.bm);
  p.tiles_n = C_out / p.bn;
  p.grid = p.tiles_m * p.tiles_n;
  return p;
}

// rows [m0, m1) and columns [n0, n1) that workgroup `block` of the plan stores (the last row tile is ragged: m1 = M)
NPVP_HD void conv3x3_tile(const Conv3x3Plan& p, int block, long long M, int& m0, int& m1, int& n0, int& n1) {
  const int tm = block / p.tiles_n, tn = block - tm * p.tiles_n;
  m0 = tm * p.bm;
  m1 = (long long)m0 + p.bm < M ? m0 + p.bm : (int)M;
  n0 = tn * p.bn;
  n1 = n0 + p.bn;
}

// ---- The transposed 3 x 3 convolution with stride 2, padding 1, output_padding 1 (the decoder's upsampling): H x W -> 2H x 2W.
// Per axis o = 2 s - 1 + k (s the source coordinate, k the kernel index, unflipped), so the output splits by parity: output coordinate
// 2 i + parity belongs to input-grid position i, and
//   parity 0 has one tap:  kernel index 1, source i;
//   parity 1 has two taps: t = 0: kernel index 2, source i;  t = 1: kernel index 0, source i + 1, or -1 (contributes 0) at the far edge.
// A pixel class (a, b) = (row parity, column parity) has ntaps(a) * ntaps(b) = 1, 2, 2 or 4 taps: 9 taps per 4 outputs.
NPVP_HD int convt3x3s2_ntaps(int parity) { return parity ? 2 : 1; }
NPVP_HD int convt3x3s2_tap(int parity, int t) { return parity ? (t ? 0 : 2) : 1; }
NPVP_HD int convt3x3s2_src(int i, int parity, int t, int extent) {
  if (parity && t) return i + 1 < extent ? i + 1 : -1;
  return i;
}

// The plan of ONE launch per transposed convolution: conv3x3_plan's tiles over M = F H W input-grid rows, once per pixel class; block b
// -> class 3 - b / p.grid (the 4-tap class (1, 1) first: the longest workgroups start first, the 1-tap class last), tile b % p.grid of
// that class.  4 * p.grid workgroups.  cls = 2 a + b.
NPVP_HD int convt3x3s2_grid(const Conv3x3Plan& p) { return 4 * p.grid; }

NPVP_HD void convt3x3s2_tile(const Conv3x3Plan& p, int block, long long M, int& cls, int& m0, int& m1, int& n0, int& n1) {
  const int q = block / p.grid;
  cls = 3 - q;
  conv3x3_tile(p, block - q * p.grid, M, m0, m1, n0, n1);
}

}  // namespace npvp
