// Counter-based attention dropout shared by the training attention kernels (attention.hip,
// attention_d64.hip, attention_f32.hip): murmur3 fmix32 (grt_common.h) of the (batch*head, query, key) coordinates
// mixed with the per-call seed. Stateless, so the forward and both backward kernels of every family
// regenerate the same mask without storing it. ops/_ref.attn_dropout_keep is the host twin and must
// agree with this file bit for bit.
#pragma once
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {

__device__ __forceinline__ uint32_t attn_dropout_hash(uint32_t seed, uint32_t bh, uint32_t q, uint32_t k) {
  uint32_t h = seed ^ (bh * 0x9E3779B1u);
  h = fmix32(h ^ (q * 0x85EBCA77u));
  return fmix32(h ^ (k * 0xC2B2AE3Du));
}
// multiplier of score (q, k): drop_scale if kept, 0 if dropped
__device__ __forceinline__ float drop_factor(const AttnParams& p, uint32_t bh, int q, int k) {
  return attn_dropout_hash(p.drop_seed, bh, (uint32_t)q, (uint32_t)k) >= p.drop_thresh ? p.drop_scale : 0.f;
}

}  // namespace grt
