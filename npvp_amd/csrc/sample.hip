// The latent sampler of the stochastic predictor, drawn S times (npvp_reparam_samples; ref/models/submodules.py:408-410,
// reparameterize: z = mu + exp(0.5 logvar) * eps with eps ~ N(0, 1), called once per forward at ref/models/Predictor.py:320-322).
//
//   z[s, i] = mu[i] + expf(0.5f * logvar[i]) * g(ctr),        ctr = (sample_base + s) * numel + i   (64 bits)
//   g(ctr)  = sqrtf(-2 * logf(u1)) * cosf(2 pi * u2)                                            (Box-Muller)
//   u1 = ((r1 >> 8) + 1) * 2^-24  in (0, 1],   r1 = rng_u32(seed, salt, 2 ctr)       (the counter hash of common.h)
//   u2 =  (r2 >> 8)      * 2^-24  in [0, 1),   r2 = rng_u32(seed, salt, 2 ctr + 1)
//
// with the precise logf / cosf / sqrtf (tests/test_hip_sampling.py restates these lines in numpy).  |g| <= sqrt(48 ln 2) = 5.77.
// The counter is the element's index in the [sample_base + s][numel] array of ALL samples, so sample sample_base + s has the same
// bits whatever S is and however a caller cuts S into chunks.  `seed` lives in device memory, as for the dropout masks: a captured
// graph sees a fresh value on every replay.
//
// One thread per four elements: mu, logvar and expf(0.5 logvar) are read / evaluated once and reused for all S draws (the loop over
// s runs inside the thread).  mu / logvar leave memory as float4; z / eps_out are stored as float4 where numel % 4 == 0 (every row
// of [S][numel] is then 16-byte aligned), as four scalar stores otherwise, and the numel % 4 trailing elements are a scalar tail.
// Plain stores, no atomics.  No amax slot: z is the `add` operand of the positional fuser, which takes none (ops.posfuse).
#include "common.h"

namespace npvp {

__device__ __forceinline__ float sample_gauss(uint64_t seed, uint32_t salt, uint64_t ctr) {
  const uint32_t r1 = rng_u32(seed, salt, 2ull * ctr), r2 = rng_u32(seed, salt, 2ull * ctr + 1ull);
  const float u1 = (float)((r1 >> 8) + 1u) * 5.9604644775390625e-8f;      // (integers up to 2^24 and the power of two: exact)
  const float u2 = (float)(r2 >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void reparam_samples_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                              float* __restrict__ z, float* __restrict__ eps_out, long long numel,
                                                              int S, long long sample_base, const unsigned long long* seedp,
                                                              unsigned int salt) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, nquad = numel >> 2;
  const unsigned long long seed = *seedp;
  if (t < nquad) {
    const long long i = 4 * t;
    const float4 m = ld4(mu + i), lv = ld4(logvar + i);
    const float sd[4] = {expf(0.5f * lv.x), expf(0.5f * lv.y), expf(0.5f * lv.z), expf(0.5f * lv.w)};
    const float mm[4] = {m.x, m.y, m.z, m.w};
    for (int s = 0; s < S; ++s) {
      const unsigned long long ctr = (unsigned long long)(sample_base + s) * (unsigned long long)numel + (unsigned long long)i;
      float e[4], zz[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { e[j] = sample_gauss(seed, salt, ctr + j); zz[j] = mm[j] + sd[j] * e[j]; }
      float* zp = z + (long long)s * numel + i;
      float* ep = eps_out ? eps_out + (long long)s * numel + i : nullptr;
      if (ALIGNED) {
        st4(zp, make_float4(zz[0], zz[1], zz[2], zz[3]));
        if (ep) st4(ep, make_float4(e[0], e[1], e[2], e[3]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { zp[j] = zz[j]; if (ep) ep[j] = e[j]; }
      }
    }
  } else if (!ALIGNED && t - nquad < (numel & 3)) {          // scalar tail: the last numel % 4 elements
    const long long i = 4 * nquad + (t - nquad);
    const float m = mu[i], sd = expf(0.5f * logvar[i]);
    for (int s = 0; s < S; ++s) {
      const float e = sample_gauss(seed, salt, (unsigned long long)(sample_base + s) * (unsigned long long)numel + (unsigned long long)i);
      z[(long long)s * numel + i] = m + sd * e;
      if (eps_out) eps_out[(long long)s * numel + i] = e;
    }
  }
}

}  // namespace npvp

using namespace npvp;

extern "C" int npvp_reparam_samples(const float* mu, const float* logvar, float* z, float* eps_out, long long numel, int S,
                                    long long sample_base, const unsigned long long* seed, unsigned int salt, hipStream_t stream) {
  NPVP_CHECK_ARG(mu && logvar && z && seed, "reparam_samples: null operand (mu, logvar, z and the device seed are required)");
  NPVP_CHECK_ARG(numel > 0 && S > 0 && sample_base >= 0, "reparam_samples: numel and S must be positive, sample_base not negative");
  NPVP_CHECK_ARG(((uintptr_t)mu % 16) == 0 && ((uintptr_t)logvar % 16) == 0 && ((uintptr_t)z % 16) == 0 && ((uintptr_t)eps_out % 16) == 0,
                 "reparam_samples: pointers must be 16-byte aligned");
  // two hash counters per draw: 2 * (sample_base + S) * numel must fit 64 bits (kept below 2^62)
  NPVP_CHECK_ARG(numel < (1ll << 40) && sample_base + S < (1ll << 20), "reparam_samples: counter range (numel < 2^40, sample_base + S < 2^20)");
  const long long threads = (numel >> 2) + (numel & 3), blocks = (threads + 255) / 256;
  NPVP_CHECK_ARG(blocks < (1ll << 31), "reparam_samples: too many elements for one launch");
  if (numel % 4 == 0)
    NPVP_LAUNCH((reparam_samples_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream, mu, logvar, z, eps_out, numel, S,
                sample_base, seed, salt);
  else
    NPVP_LAUNCH((reparam_samples_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream, mu, logvar, z, eps_out, numel, S,
                sample_base, seed, salt);
  NPVP_CHECK_LAUNCH();
  return NPVP_OK;
}
