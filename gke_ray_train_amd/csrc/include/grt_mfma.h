// v_mfma_f32_32x32x16_bf16 and the layout of its 32 x 32 fp32 accumulator (cdna_hip_programming.md
// §3), shared by the attention and LoRA kernels.
#pragma once
#include "grt_common.h"

namespace grt {

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// accumulator element r of lane half h (lane >> 5) holds row (r & 3) + 8 (r >> 2) + 4 h of the
// 32-row tile, column lane & 31 (the same map for the fp32 32x32x2 MFMA of attention_f32.hip)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// accumulator elements base .. base + 7 as the bf16 operand of the next MFMA
__device__ __forceinline__ bf16x8 pack8(const f32x16& x, int base) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = static_cast<bf16>(x[base + j]);
  return r;
}

}  // namespace grt
