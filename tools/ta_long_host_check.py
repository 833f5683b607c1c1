"""Host emulation of the temporal attention kernels (npvp_amd/csrc/ae_temporal.hip), the key-tiled ones above all: the kernel source
compiled for the CPU as it stands (the file's text after its #include line, behind a prelude that supplies float4, threadIdx / blockIdx,
__syncthreads as a barrier of 256 host threads, and NPVP_LAUNCH as a loop over the grid, one block at a time) into a stand-alone
program built with -fsanitize=address,undefined.  The program calls the C entry points themselves - so the host-side checks, the tile
choice and the LDS sizes are the library's - on exact-size heap buffers: q / k / v / go / o / dq / dk / dv each with a leading dimension
of its own, outputs NaN-filled, the LDS array poisoned past the size the launch asked for.  Per case it prints rel-L2 against float64
of o, lse, dq, dk, dv and `bad`: output elements not written, pad columns written, non-finite results, a D that moved at T <= 32.
No GPU, nothing loaded into Python.  Usage: python tools/ta_long_host_check.py [--keep DIR]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "npvp_amd", "csrc", "ae_temporal.hip")

PRELUDE = r"""
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <thread>
#include <vector>
#include <sanitizer/asan_interface.h>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __shared__
#define __launch_bounds__(n)
#define NPVP_OK 0
#define NPVP_ERR_ARG (-1)
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline float4 ld4(const float* p) { float4 v; memcpy(&v, p, 16); if ((uintptr_t)p & 15) abort(); return v; }
static inline void st4(float* p, float4 v) { if ((uintptr_t)p & 15) abort(); memcpy(p, &v, 16); }
struct dim3 { unsigned x; dim3(unsigned x_ = 1) : x(x_) {} };
typedef void* hipStream_t;
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static pthread_barrier_t g_bar;
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
alignas(16) float4 ta_lds4[65536 / 16];                                 /* the block's LDS: the limit of one workgroup */
static char g_err[512];
static void npvp_set_error(const char* m) { snprintf(g_err, sizeof g_err, "%s", m); }
static long g_launches = 0, g_lds_max = 0;
#define NPVP_CHECK_ARG(cond, msg) do { if (!(cond)) { npvp_set_error(msg); return NPVP_ERR_ARG; } } while (0)
#define NPVP_CHECK_LAUNCH() do { } while (0)
template <class K, class... Args>
static void emu_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, Args... args) {
  if (block.x != 256 || lds > sizeof ta_lds4) { fprintf(stderr, "launch: block %u, lds %zu\n", block.x, lds); abort(); }
  ++g_launches;
  if ((long)lds > g_lds_max) g_lds_max = (long)lds;
  ASAN_UNPOISON_MEMORY_REGION(ta_lds4, sizeof ta_lds4);
  for (size_t i = 0; i < sizeof ta_lds4 / 4; ++i) ((float*)ta_lds4)[i] = NAN;   /* LDS is not initialised */
  ASAN_POISON_MEMORY_REGION((char*)ta_lds4 + lds, sizeof ta_lds4 - lds);
  std::vector<std::thread> th;
  for (int t = 0; t < 256; ++t)
    th.emplace_back([=] {
      for (unsigned b = 0; b < grid.x; ++b) {
        threadIdx.x = t; blockIdx.x = (int)b;
        kernel(args...);
        pthread_barrier_wait(&g_bar);
      }
    });
  for (auto& x : th) x.join();
  ASAN_UNPOISON_MEMORY_REGION(ta_lds4, sizeof ta_lds4);
}
#define NPVP_LAUNCH(kernel, ...) emu_launch(kernel, __VA_ARGS__)
"""

MAIN = r"""
struct Buf {                                   /* rows x ld floats on the heap, exactly */
  float* p; long rows; int ld, cols;
  Buf(long r, int l, int c, float fill) : rows(r), ld(l), cols(c) { if (posix_memalign((void**)&p, 16, (size_t)r * l * 4)) abort(); for (long i = 0; i < r * l; ++i) p[i] = fill; }
  ~Buf() { free(p); }
  float& at(long r, int c) { return p[r * ld + c]; }
};
static uint64_t g_seed;
static float rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; double s = 0; for (int i = 0; i < 4; ++i) { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; s += (double)(g_seed >> 11) / 9007199254740992.0; } return (float)((s - 2.0) * 1.7320508); }
static double rel(const std::vector<double>& want, Buf& got, long* bad) {
  double num = 0, den = 0;
  for (long r = 0; r < got.rows; ++r) {
    for (int c = 0; c < got.cols; ++c) { const double g = got.at(r, c), w = want[r * got.cols + c]; if (!isfinite(g)) ++*bad; num += (g - w) * (g - w); den += w * w; }
    for (int c = got.cols; c < got.ld; ++c) if (!isnan(got.at(r, c))) ++*bad;         /* pad columns keep their NaN */
  }
  return sqrt(num / (den > 0 ? den : 1));
}
static int run(int A, int V, int N, int T, int HW, int plant) {
  const long R = (long)N * T * HW;
  Buf q(R, A + 4, A, NAN), k(R, A + 8, A, NAN), v(R, V + 4, V, NAN), go(R, V + 8, V, NAN);
  Buf o(R, V + 12, V, NAN), dq(R, A, A, NAN), dk(R, A + 12, A, NAN), dv(R, V, V, NAN), lse(R, 1, 1, NAN), D(2 * R, 1, 1, -7.f);
  g_seed = 1234567 + A * 131 + T * 7 + HW;
  for (long r = 0; r < R; ++r) {
    for (int c = 0; c < A; ++c) { q.at(r, c) = rnd() * 1.5f / sqrtf((float)A); k.at(r, c) = rnd(); }
    for (int c = 0; c < V; ++c) { v.at(r, c) = rnd(); go.at(r, c) = rnd(); }
  }
  if (plant) {                                   /* the max arrives in the last key tile / sits in the first */
    auto row = [&](int n, int t, int p) { return ((long)n * T + t) * HW + p; };
    for (int c = 0; c < A; ++c) { q.at(row(0, 3, 1), c) = k.at(row(0, T - 1, 1), c) = sqrtf(120.f / A); q.at(row(1, T - 5, 2), c) = k.at(row(1, 0, 2), c) = sqrtf(120.f / A); }
  }
  std::vector<double> wo(R * V), wl(R), wdq(R * A), wdk(R * A, 0.0), wdv(R * V, 0.0);
  std::vector<double> P(T), dP(T);
  for (int n = 0; n < N; ++n) for (int p = 0; p < HW; ++p) for (int i = 0; i < T; ++i) {
    const long ri = ((long)n * T + i) * HW + p;
    double mx = -1e300, l = 0, Dd = 0;
    for (int j = 0; j < T; ++j) { const long rj = ((long)n * T + j) * HW + p; double s = 0; for (int c = 0; c < A; ++c) s += (double)q.at(ri, c) * k.at(rj, c); P[j] = s; mx = s > mx ? s : mx; }
    for (int j = 0; j < T; ++j) { P[j] = exp(P[j] - mx); l += P[j]; }
    wl[ri] = mx + log(l);
    for (int c = 0; c < V; ++c) wo[ri * V + c] = 0;
    for (int j = 0; j < T; ++j) {
      const long rj = ((long)n * T + j) * HW + p; P[j] /= l; double d = 0;
      for (int c = 0; c < V; ++c) { wo[ri * V + c] += P[j] * v.at(rj, c); d += (double)go.at(ri, c) * v.at(rj, c); wdv[rj * V + c] += P[j] * go.at(ri, c); }
      dP[j] = d; Dd += P[j] * d;
    }
    for (int c = 0; c < A; ++c) wdq[ri * A + c] = 0;
    for (int j = 0; j < T; ++j) {
      const long rj = ((long)n * T + j) * HW + p; const double dS = P[j] * (dP[j] - Dd);
      for (int c = 0; c < A; ++c) { wdq[ri * A + c] += dS * k.at(rj, c); wdk[rj * A + c] += dS * q.at(ri, c); }
    }
  }
  g_launches = 0; g_lds_max = 0;
  int rc = npvp_temporal_attn_long_fwd(q.p, q.ld, k.p, k.ld, v.p, v.ld, o.p, o.ld, lse.p, N, T, HW, A, V, nullptr);
  if (!rc) rc = npvp_temporal_attn_long_bwd(q.p, q.ld, k.p, k.ld, v.p, v.ld, go.p, go.ld, lse.p, D.p, dq.p, dq.ld, dk.p, dk.ld, dv.p, dv.ld, N, T, HW, A, V, nullptr);
  if (rc) { printf("(%d,%d) N=%d T=%d HW=%d: rc %d %s\n", A, V, N, T, HW, rc, g_err); return 1; }
  long bad = 0;
  const double eo = rel(wo, o, &bad), el = rel(wl, lse, &bad), eq = rel(wdq, dq, &bad), ek = rel(wdk, dk, &bad), ev = rel(wdv, dv, &bad);
  for (long i = 0; i < 2 * R; ++i) if (T <= 32 ? D.p[i] != -7.f : !isfinite(D.p[i]) || D.p[i] == -7.f) ++bad;
  if (g_launches != (T <= 32 ? 2 : 3)) ++bad;
  printf("(%2d,%3d) N=%d T=%3d HW=%3d %s o %.2e lse %.2e dq %.2e dk %.2e dv %.2e  launches %ld lds %ld  bad %ld\n", A, V, N, T, HW,
         plant ? "planted" : "       ", eo, el, eq, ek, ev, g_launches, g_lds_max, bad);
  return bad != 0 || !(eo < 1e-5 && el < 1e-5 && eq < 1e-5 && ek < 1e-5 && ev < 1e-5);
}
int main() {
  pthread_barrier_init(&g_bar, nullptr, 256);
  static const int cases[][6] = {
    {8, 32, 2, 33, 5, 0}, {16, 64, 2, 33, 5, 0}, {32, 128, 2, 33, 5, 0}, {64, 256, 2, 33, 5, 0},
    {8, 32, 2, 64, 5, 0}, {64, 256, 2, 64, 5, 0}, {16, 64, 2, 65, 5, 0}, {32, 128, 2, 97, 5, 0}, {8, 32, 2, 40, 5, 0}, {8, 32, 2, 50, 5, 0},
    {8, 32, 2, 33, 1, 0}, {8, 32, 2, 33, 3, 0}, {8, 32, 2, 33, 4, 0}, {8, 32, 2, 33, 5, 0}, {8, 32, 2, 33, 6, 0}, {8, 32, 2, 33, 7, 0},
    {8, 32, 2, 33, 19, 0}, {8, 32, 2, 33, 27, 0}, {64, 256, 2, 33, 3, 0},
    {16, 64, 2, 40, 5, 1}, {32, 128, 2, 40, 6, 0}, {8, 32, 2, 33, 17, 0}, {8, 32, 2, 9, 5, 0}, {64, 256, 1, 32, 3, 0}, {8, 32, 1, 1, 3, 0},
  };
  int fails = 0;
  for (auto& c : cases) fails += run(c[0], c[1], c[2], c[3], c[4], c[5]);
  /* refusals: made before any launch */
  float x[4];
  g_launches = 0;
  if (npvp_temporal_attn_long_fwd(x, 48, x, 48, x, 48, x, 32, x, 2, 0, 5, 8, 32, nullptr) != -1 || !strstr(g_err, "T = 0")) ++fails;
  if (npvp_temporal_attn_long_bwd(x, 48, x, 48, x, 48, x, 32, x, nullptr, x, 48, x, 48, x, 48, 2, 40, 5, 8, 32, nullptr) != -1 || !strstr(g_err, "null buffer D")) ++fails;
  if (g_launches) ++fails;
  printf(fails ? "FAILED: %d\n" : "all cases within 1e-5 of float64, bad = 0 (%d failures)\n", fails);
  return fails != 0;
}
"""


def main():
    text = open(SRC).read()
    body = text.split('#include "common.h"', 1)[1].replace("#include <stdio.h>", "")
    body = body.replace("extern __shared__ float4 ta_lds4[];", "")
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as td:
        td = keep or td
        os.makedirs(td, exist_ok=True)
        src, exe = os.path.join(td, "ta_long_host_check.cpp"), os.path.join(td, "ta_long_host_check")
        with open(src, "w") as f:
            f.write(PRELUDE + body + MAIN)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                        "-I" + os.path.dirname(SRC), src, "-o", exe], check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
