// The two-term fp16 split of the "f16x3" arithmetic (gemm_f16.hip, conv3x3.hip): one definition for every kernel that stages an
// fp32 operand as scaled fp16 planes.
#pragma once
#include "common.h"

namespace npvp {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// x, s -> (hi, lo) of x s:  hi = rne_f16(x s),  lo = rne_f16(x s - hi).  TWO VALU instructions per element, the mixed-precision FMAs
// (v_fma_mixlo_f16 / v_fma_mixhi_f16: an fp32 FMA whose operands may be fp16 halves and whose result is rounded into one half of the
// destination): hi = mix(x, s, 0), lo = mix(x, s, -hi).  Both FMAs are exact before the conversion (s is a power of two; x s - hi
// has at most 13 significant bits), so the halves are bit for bit those of "scale, convert, convert back, subtract, convert"
// (tools/f16_split_check.hip runs both forms over random and edge-case words on the GPU) - which cost 3 VALU per element as the
// compiler's best (pk_mul, cvt_pk, 2 cvt back, pk_fma, cvt_pk per pair; 8 - 9 in the scalar form of round 3).  Every VALU
// instruction of the K loop costs its 4 cycles on top of the MFMAs' (profiles/r03_gemm_f16_latency.txt); the split was 28 of the
// forward loop's 36 per step and ~76 of the weight-gradient loop's.
__device__ __forceinline__ void split_f16_scaled(const f32x4 v, const float s, f16x4& hi, f16x4& lo) {
  unsigned int h01, h23, l01, l23;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h01) : "v"(v[0]), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h23) : "v"(v[2]), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h01) : "v"(v[1]), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h23) : "v"(v[3]), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l01) : "v"(v[0]), "v"(s), "v"(h01));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l23) : "v"(v[2]), "v"(s), "v"(h23));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l01) : "v"(v[1]), "v"(s), "v"(h01));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l23) : "v"(v[3]), "v"(s), "v"(h23));
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 hp = {h01, h23}, lp = {l01, l23};
  hi = __builtin_bit_cast(f16x4, hp);
  lo = __builtin_bit_cast(f16x4, lp);
}

}  // namespace npvp
