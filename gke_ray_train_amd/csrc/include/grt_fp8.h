// OCP e4m3fn helpers of the fp8 KV cache (kv_fp8.hip, decode_attention.hip). The format is defined
// by ops/_ref.py::kv_fp8_quantize: one fp32 scale = max|x| / 448 per head vector (1 for a zero
// vector), code = x / scale clamped to +-448 and rounded to nearest-even e4m3fn.
//
// The encode is exact integer arithmetic (the append is off the hot path, and the cache contents
// then do not depend on how a conversion instruction treats ties, subnormals or saturation); the
// decode in the attention loop is gfx950's own convert, v_cvt_pk_f32_fp8 (OCP on gfx950), which is
// exact for every finite code.
#pragma once
#include "grt_common.h"

namespace grt {

constexpr float kFp8Max = 448.f;  // code 126, the largest finite e4m3fn value

// |y| <= 448 (the caller clamps) -> e4m3fn code, round to nearest even. Below the smallest normal
// 2^-6 the codes are the multiples of 2^-9 (code 8 is 2^-6 itself); from there on the code is the
// fp32 exponent and the top 3 mantissa bits, re-biased by (127 - 7) << 3 = 960 after rounding the
// 20 bits below them (a carry out of the mantissa moves into the exponent, as it should).
__host__ __device__ __forceinline__ uint32_t fp8_e4m3_encode(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t mag = u & 0x7fffffffu;
  const float a = __builtin_bit_cast(float, mag);
  uint32_t code;
  if (a < 0.015625f) {
    code = (uint32_t)__builtin_rintf(a * 512.f);
  } else {
    code = ((mag + 0x7ffffu + ((mag >> 20) & 1u)) >> 20) - 960u;
  }
  return ((u >> 24) & 0x80u) | (code & 0x7fu);
}

// scale of a head vector from its max |x|
__host__ __device__ __forceinline__ float fp8_scale(float amax) { return amax == 0.f ? 1.f : amax / kFp8Max; }

// x / scale, clamped, encoded
__host__ __device__ __forceinline__ uint32_t fp8_quantize(float x, float scale) {
  float y = x / scale;
  y = y > kFp8Max ? kFp8Max : y;
  y = y < -kFp8Max ? -kFp8Max : y;
  return fp8_e4m3_encode(y);
}

// 8 codes held as two dwords -> fp32 (the body exists in the device pass only: the host pass has
// no such builtin and never calls it)
__device__ __forceinline__ void fp8x8_to_f32(uint32_t lo, uint32_t hi, float (&f)[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
  f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
#else
  (void)lo; (void)hi; (void)f;
#endif
}

}  // namespace grt
