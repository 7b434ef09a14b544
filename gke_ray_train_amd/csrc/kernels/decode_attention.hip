// Split-K attention for the decode step (one new query token per sequence), bf16, head_dim 128 or 64.
//
// Reference role: the KV-cache decode of HF ``generate`` in the inference comparison
// (reference ray-jobs/fine_tune_llama_ray.py:138-146). With Sq = 1 the
// training flash kernel runs one workgroup per (batch, query head) that walks all cached keys in
// sequence — 32 workgroups for Llama-3.1-8B at batch 1, ~24 µs per layer. Here the cached keys of
// each (batch, kv head) are split over NS workgroups (grid ~512) that each produce a partial
// (max, sum, unnormalised output) for every query head of the GQA group; a second tiny kernel
// merges the NS partials (log-sum-exp combine) and writes bf16.
//
// Lane mapping: D / 8 lanes per key (8 of the D dims each, one 16-byte load of K and of V), so at
// head_dim 128 16 lanes per key, 4 keys per wave per step, 16 keys per workgroup per step, and at
// head_dim 64 (Llama-3.2-1B) 8 lanes per key, 8 keys per wave, 32 keys per workgroup per step; the
// GQA group's query rows stay in registers (fp32). Partial states of the key-lane-groups of a wave
// merge with shuffles (lane offsets D / 8 .. 32), the 4 waves through LDS. Empty splits (keys
// beyond the valid length) emit max = -inf, sum = 0. The kernels are templates on D; every
// constant below is the head_dim-128 kernel's own at D = 128. At head_dim 64 a short cache
// (Sk <= kSingleSplitKeys) is one split that writes the output itself: below that length the
// second launch costs more than the splits save.
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

template <int D, int G>
__global__ __launch_bounds__(256) void attn_decode_split_kernel(const AttnDecodeParams p) {
  constexpr int kLanes = D / 8;           // lanes per key
  constexpr int kWaveKeys = 64 / kLanes;  // keys per wave per step
  constexpr int kStep = 4 * kWaveKeys;    // keys per workgroup per step
  __shared__ float sm_m[4][G], sm_l[4][G];
  __shared__ float sm_o[4][G][D];
  const int bh = blockIdx.x, split = blockIdx.y;
  const int b = bh / p.Hkv, hkv = bh % p.Hkv;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane / kLanes, c = lane % kLanes;  // key lane-group, 16-byte chunk of the head dim
  int len = p.Sk;
  if (p.seqlens_k) len = min(len, p.seqlens_k[b]);
  const int per = ((len + p.NS - 1) / p.NS + kStep - 1) / kStep * kStep;
  const int k0 = split * per, k1 = min(len, k0 + per);

  const bf16* Kb = (const bf16*)p.k + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs + c * 8;
  const bf16* Vb = (const bf16*)p.v + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs + c * 8;
  // the K / V stream is pipelined one step ahead, and its first loads are issued before the query
  // loads, so the two dependent round trips at the start overlap (most splits are 1-2 steps long)
  int j = k0 + wave * kWaveKeys + grp;
  u32x4 kraw{}, vraw{};
  if (j < k1) {
    kraw = *reinterpret_cast<const u32x4*>(Kb + (int64_t)j * p.k_ss);
    vraw = *reinterpret_cast<const u32x4*>(Vb + (int64_t)j * p.v_ss);
  }
  float q[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16* qp = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)(hkv * G + g) * p.q_hs + c * 8;
    bf16x8_to_f32(*reinterpret_cast<const u32x4*>(qp), q[g]);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[g][i] *= p.scale_log2;  // scores in log2 units
  }
  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[g][i] = 0.f;
  }
  for (; j < k1; j += kStep) {
    float kf[8], vf[8];
    bf16x8_to_f32(kraw, kf);
    bf16x8_to_f32(vraw, vf);
    if (j + kStep < k1) {
      kraw = *reinterpret_cast<const u32x4*>(Kb + (int64_t)(j + kStep) * p.k_ss);
      vraw = *reinterpret_cast<const u32x4*>(Vb + (int64_t)(j + kStep) * p.v_ss);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(q[g][i], kf[i], s);
#pragma unroll
      for (int off = kLanes / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
      const float mn = fmaxf(m[g], s);
      const float a = fast_exp2(m[g] - mn), e = fast_exp2(s - mn);
      l[g] = l[g] * a + e;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[g][i] = fmaf(o[g][i], a, e * vf[i]);
      m[g] = mn;
    }
  }
  // merge the key lane-groups of the wave (lanes c, c + D/8, c + 2 D/8, ... hold the same dims)
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int off = kLanes; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
      const float mn = fmaxf(m[g], m2);
      const float a = mn == -INFINITY ? 0.f : fast_exp2(m[g] - mn);
      const float a2 = mn == -INFINITY ? 0.f : fast_exp2(m2 - mn);
      l[g] = l[g] * a + l2 * a2;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[g][i] = o[g][i] * a + __shfl_xor(o[g][i], off, 64) * a2;
      m[g] = mn;
    }
    if (grp == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wave][g][c * 8 + i] = o[g][i];
      if (c == 0) { sm_m[wave][g] = m[g]; sm_l[wave][g] = l[g]; }
    }
  }
  __syncthreads();
  // merge the 4 waves: thread t handles (g, d) pairs
  for (int idx = threadIdx.x; idx < G * D; idx += 256) {
    const int g = idx / D, d = idx % D;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mm = fmaxf(mm, sm_m[w][g]);
    float ll = 0.f, oo = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float a = mm == -INFINITY ? 0.f : fast_exp2(sm_m[w][g] - mm);
      ll += sm_l[w][g] * a;
      oo += sm_o[w][g][d] * a;
    }
    if constexpr (D == 64) {
      if (p.NS == 1) {  // short cache, one split: this is the whole softmax, no combine launch
        bf16* op = (bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)(hkv * G + g) * p.o_hs + d;
        *op = static_cast<bf16>(ll > 0.f ? oo / ll : 0.f);
        continue;
      }
    }
    const int64_t slot = ((int64_t)(b * p.Hq + hkv * G + g) * p.NS + split);
    p.part_o[slot * D + d] = oo;
    if (d == 0) { p.part_m[slot] = mm; p.part_l[slot] = ll; }
  }
}

// One workgroup per (batch, query head), one thread per head dim (D threads). The NS <= 64 partial
// states are loaded by the lanes of wave 0 in parallel (max / weight / sum by butterflies, weights to LDS),
// then every thread sums its dimension over the splits with independent loads — two dependent
// round trips instead of a serial NS-long chain.
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const AttnDecodeParams p) {
  __shared__ float wts[64];
  __shared__ float lsum;
  const int bhq = blockIdx.x, d = threadIdx.x;
  const int b = bhq / p.Hq, hq = bhq % p.Hq;
  const int64_t base = (int64_t)bhq * p.NS;
  if (threadIdx.x < 64) {
    const int s = threadIdx.x;
    const bool ok = s < p.NS;
    const float ms = ok ? p.part_m[base + s] : -INFINITY;
    const float ls = ok ? p.part_l[base + s] : 0.f;
    float mm = ms;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mm = fmaxf(mm, __shfl_xor(mm, off, 64));
    const float a = (mm == -INFINITY || !ok) ? 0.f : fast_exp2(ms - mm);
    float ll = ls * a;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ll += __shfl_xor(ll, off, 64);
    wts[s] = a;
    if (s == 0) lsum = ll;
  }
  __syncthreads();
  const float* po = p.part_o + base * D + d;
  float oo = 0.f;
#pragma unroll 8
  for (int s = 0; s < p.NS; ++s) oo = fmaf(po[(int64_t)s * D], wts[s], oo);
  const float ll = lsum;
  bf16* op = (bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)hq * p.o_hs + d;
  *op = static_cast<bf16>(ll > 0.f ? oo / ll : 0.f);
}

template <int D>
void launch_decode(const AttnDecodeParams& p, hipStream_t s) {
  const dim3 g1((unsigned)(p.B * p.Hkv), (unsigned)p.NS);
  const int G = p.Hq / p.Hkv;
  switch (G) {
    case 1: hipLaunchKernelGGL((attn_decode_split_kernel<D, 1>), g1, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL((attn_decode_split_kernel<D, 2>), g1, dim3(256), 0, s, p); break;
    case 4: hipLaunchKernelGGL((attn_decode_split_kernel<D, 4>), g1, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((attn_decode_split_kernel<D, 8>), g1, dim3(256), 0, s, p); break;
  }
  if (D == 64 && p.NS == 1) return;  // the split kernel wrote the output itself
  hipLaunchKernelGGL(attn_decode_combine_kernel<D>, dim3((unsigned)(p.B * p.Hq)), dim3(D), 0, s, p);
}

// head_dim 64: up to this many cached keys run as ONE split whose kernel normalises and writes the
// bf16 output itself, with no combine launch. Llama-3.2-1B geometry, batch 1, back-to-back calls:
// one launch 5.2 / 6.6 / 8.5 / 9.5 us at Sk 32 / 128 / 256 / 320 against 8.8-9.4 us for split +
// combine at every such Sk and 5.9 / 7.1 / 10.9 / 12.9 us for the flash forward kernel
// (profiles/decode_d64.md)
constexpr int kSingleSplitKeys = 256;

}  // namespace

// splits per (batch, kv head): ~512 workgroups in all, at least one workgroup step of keys (16 at
// head_dim 128, 32 at head_dim 64) per split, at most 64 (the combine kernel's one wave of partials)
int attn_decode_splits(int B, int Hkv, int Sk, int head_dim) {
  if (head_dim == 64 && Sk <= kSingleSplitKeys) return 1;
  const int step = 4 * (64 / (head_dim / 8));
  int ns = (512 + B * Hkv - 1) / (B * Hkv);
  const int max_ns = (Sk + step - 1) / step;
  if (ns > max_ns) ns = max_ns;
  if (ns > 64) ns = 64;
  return ns < 1 ? 1 : ns;
}

void attn_decode(const AttnDecodeParams& p, hipStream_t s) { launch_decode<128>(p, s); }

void attn_decode_d64(const AttnDecodeParams& p, hipStream_t s) { launch_decode<64>(p, s); }

}  // namespace grt
