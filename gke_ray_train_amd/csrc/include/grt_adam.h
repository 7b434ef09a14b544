// The AdamW element update and the stochastic-rounding stream shared by the optimizer kernels
// (optim.hip: fp32 moments; adamw8.hip: 8-bit block-quantised moments), so every variant rounds alike.
#pragma once
#include "grt_common.h"

namespace grt {

// fp32 -> bf16 with stochastic rounding: add 16 random bits below the bf16 mantissa, truncate.
__device__ __forceinline__ bf16 sr_bf16(float x, uint32_t r16) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return static_cast<bf16>(x);  // inf / nan unchanged
  const uint32_t t = (u + r16) & 0xffff0000u;
  return static_cast<bf16>(__uint_as_float(t));  // exact: the low 16 bits are zero
}

// One AdamW element update with its fused multiply-adds spelled out, so every kernel variant (8- /
// 4-wide, scalar tail, transposing) rounds identically whatever the compiler would contract.
// FAST (default; GRT_ADAMW_FASTMATH=0 -> the IEEE forms): v_sqrt_f32 and v_rcp_f32 (1 ulp each)
// instead of the correctly rounded sqrtf / division, whose expansions (denormal scaling, div_scale /
// div_fmas / div_fixup) made up over a third of the kernel's ~57 VALU instructions per element. The
// step is power-capped (1.39 kW on every sample of the headline step, profiles/r6_power.md), so the
// update's instruction energy beside the forward costs step time even though the pass is HBM-bound.
template <bool FAST>
__device__ __forceinline__ float adam_elem(float p, float gf, float& m, float& v, float b1, float b2, float rbc2,
                                           float eps, float decay, float step) {
  m = fmaf(b1, m, (1.f - b1) * gf);
  v = fmaf(b2, v, (1.f - b2) * gf * gf);
  if constexpr (FAST) {
    const float denom = fmaf(__builtin_amdgcn_sqrtf(v), rbc2, eps);
    return fmaf(-step * m, __builtin_amdgcn_rcpf(denom), p * decay);
  } else {
    const float denom = fmaf(sqrtf(v), rbc2, eps);
    return fmaf(p, decay, -(step * m / denom));
  }
}

// 16 random bits per element for stochastic rounding, 4 elements at a time (element base4 + k in
// bits 16k .. 16k + 15), keyed by (step, flat element index): FAST = one 32-bit fmix per element
// pair; otherwise one 64-bit splitmix per 4 elements.
template <bool FAST>
__device__ __forceinline__ uint64_t sr_bits4(uint64_t srkey, uint64_t base4) {
  if constexpr (FAST) {
    const uint64_t pr = base4 >> 1;
    const uint32_t k = (uint32_t)srkey ^ ((uint32_t)(pr >> 32) * 0x9E3779B1u);
    return (uint64_t)fmix32(k ^ (uint32_t)pr) | ((uint64_t)fmix32(k ^ (uint32_t)(pr + 1)) << 32);
  } else {
    return hash_u64(srkey ^ (base4 >> 2));
  }
}

}  // namespace grt
