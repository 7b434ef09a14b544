// Split-K attention for the decode step, bf16 (or an fp8 cache, below), head_dim 128 or 64: one new query token per sequence,
// or the 2-4 query tokens of a speculative verify step.
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
//
// The split kernel is also a template on TT, the query tokens a workgroup handles. TT = 1 is the
// decode step. The verify step of speculative decoding has T = 2..4 query tokens per sequence, the
// last T keys of the row being their own: query token t of row b attends keys
// [0, len_b - (T - 1 - t)), len_b the valid keys including all T new ones. Split plan, lane mapping
// and partial-state contract are the same (the splits cover [0, len_b)); a workgroup keeps
// R = G * TT query rows in registers (TT tokens of the GQA group), so every K / V element is loaded
// once for all of them, and a row skips the keys at or past its own length. TT = T up to R = 16
// rows (q and o are 8 fp32 registers per row each); G = 8 with T = 3 or 4 would need 24 / 32 rows,
// more than the 512-register file of a 256-thread workgroup holds without scratch, so those two
// cases run TT = 2 tokens per workgroup and tile the tokens over blockIdx.z (K / V are then read
// twice). Partials are [B, T, Hq, NS].
//
// The kernel is last a template on KT, the cache element: bf16, or uint8_t for the fp8 cache (OCP
// e4m3fn codes with one fp32 scale per (key, kv head); kv_fp8.hip writes it). The lane mapping is
// the same, so K and V are one 8-byte load per lane, converted by v_cvt_pk_f32_fp8; the two scales
// of a key are loaded by all its lanes from one address and prefetched with the codes. The K scale
// multiplies the score after the lane reduction and the V scale the weight e of the key before
// the output FMAs (the sum l keeps e itself), so no element is scaled on its own. All of it is
// behind the compile-time KT: the bf16 instantiations carry none of it.
#include <type_traits>

#include "grt_common.h"
#include "grt_fp8.h"
#include "grt_kernels.h"

namespace grt {
namespace {

// Everything that exists only for TT > 1 (token tile, per-row key limit, token terms of the
// addresses) is behind the compile-time TT, so TT = 1 carries none of it.
template <int D, int G, int TT, typename KT>
__global__ __launch_bounds__(256) void attn_decode_split_kernel(const AttnDecodeParams p) {
  constexpr bool kFp8 = sizeof(KT) == 1;
  using Raw = std::conditional_t<kFp8, uint2, u32x4>;  // 8 cache elements of a lane
  constexpr int kLanes = D / 8;           // lanes per key
  constexpr int kWaveKeys = 64 / kLanes;  // keys per wave per step
  constexpr int kStep = 4 * kWaveKeys;    // keys per workgroup per step
  constexpr int R = G * TT;  // row r: token t0 + r / G, query head hkv * G + r % G
  __shared__ float sm_m[4][R], sm_l[4][R];
  __shared__ float sm_o[4][R][D];
  const int bh = blockIdx.x, split = blockIdx.y;
  const int t0 = TT > 1 ? blockIdx.z * TT : 0;
  const int b = bh / p.Hkv, hkv = bh % p.Hkv;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane / kLanes, c = lane % kLanes;  // key lane-group, 16-byte chunk of the head dim
  int len = p.Sk;
  if (p.seqlens_k) len = min(len, p.seqlens_k[b]);
  const int per = ((len + p.NS - 1) / p.NS + kStep - 1) / kStep * kStep;
  const int k0 = split * per, k1 = min(len, k0 + per);

  const KT* Kb = (const KT*)p.k + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs + c * 8;
  const KT* Vb = (const KT*)p.v + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs + c * 8;
  [[maybe_unused]] const float* Ksb = nullptr;
  [[maybe_unused]] const float* Vsb = nullptr;
  [[maybe_unused]] float ksn = 0.f, vsn = 0.f;  // the scales of the key in kraw / vraw
  if constexpr (kFp8) {
    Ksb = p.k_scale + (int64_t)b * p.ksc_bs + (int64_t)hkv * p.ksc_hs;
    Vsb = p.v_scale + (int64_t)b * p.vsc_bs + (int64_t)hkv * p.vsc_hs;
  }
  // the K / V stream is pipelined one step ahead, and its first loads are issued before the query
  // loads, so the two dependent round trips at the start overlap (most splits are 1-2 steps long)
  int j = k0 + wave * kWaveKeys + grp;
  Raw kraw{}, vraw{};
  if (j < k1) {
    kraw = *reinterpret_cast<const Raw*>(Kb + (int64_t)j * p.k_ss);
    vraw = *reinterpret_cast<const Raw*>(Vb + (int64_t)j * p.v_ss);
    if constexpr (kFp8) {
      ksn = Ksb[(int64_t)j * p.ksc_ss];
      vsn = Vsb[(int64_t)j * p.vsc_ss];
    }
  }
  float q[R][8];
  int rlen[TT];  // TT > 1: keys token t0 + tt sees; 0 for a token past T (last tile of an uneven tiling)
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) rlen[tt] = t0 + tt < p.T ? len - (p.T - 1 - (t0 + tt)) : 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = TT > 1 ? min(t0 + r / G, p.T - 1) : 0;  // a token past T reads token T - 1's q and uses none of it
    const bf16* qp = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)t * p.q_ts +
                     (int64_t)(hkv * G + r % G) * p.q_hs + c * 8;
    bf16x8_to_f32(*reinterpret_cast<const u32x4*>(qp), q[r]);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[r][i] *= p.scale_log2;  // scores in log2 units
  }
  float m[R], l[R], o[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[r][i] = 0.f;
  }
  for (; j < k1; j += kStep) {
    float kf[8], vf[8];
    [[maybe_unused]] const float ks = ksn, vs = vsn;
    if constexpr (kFp8) {
      fp8x8_to_f32(kraw.x, kraw.y, kf);
      fp8x8_to_f32(vraw.x, vraw.y, vf);
    } else {
      bf16x8_to_f32(kraw, kf);
      bf16x8_to_f32(vraw, vf);
    }
    if (j + kStep < k1) {
      kraw = *reinterpret_cast<const Raw*>(Kb + (int64_t)(j + kStep) * p.k_ss);
      vraw = *reinterpret_cast<const Raw*>(Vb + (int64_t)(j + kStep) * p.v_ss);
      if constexpr (kFp8) {
        ksn = Ksb[(int64_t)(j + kStep) * p.ksc_ss];
        vsn = Vsb[(int64_t)(j + kStep) * p.vsc_ss];
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(q[r][i], kf[i], s);
#pragma unroll
      for (int off = kLanes / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
      if constexpr (kFp8) s *= ks;
      // one token sees every key of its split; the limit of a row of several is uniform over the
      // lanes of a key, and the shuffles above stay outside it
      if (TT == 1 || j < rlen[r / G]) {
        const float mn = fmaxf(m[r], s);
        const float a = fast_exp2(m[r] - mn), e = fast_exp2(s - mn);
        l[r] = l[r] * a + e;
        if constexpr (kFp8) {
          const float ev = e * vs;
#pragma unroll
          for (int i = 0; i < 8; ++i) o[r][i] = fmaf(o[r][i], a, ev * vf[i]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) o[r][i] = fmaf(o[r][i], a, e * vf[i]);
        }
        m[r] = mn;
      }
    }
  }
  // merge the key lane-groups of the wave (lanes c, c + D/8, c + 2 D/8, ... hold the same dims)
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int off = kLanes; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(m[r], off, 64), l2 = __shfl_xor(l[r], off, 64);
      const float mn = fmaxf(m[r], m2);
      const float a = mn == -INFINITY ? 0.f : fast_exp2(m[r] - mn);
      const float a2 = mn == -INFINITY ? 0.f : fast_exp2(m2 - mn);
      l[r] = l[r] * a + l2 * a2;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[r][i] = o[r][i] * a + __shfl_xor(o[r][i], off, 64) * a2;
      m[r] = mn;
    }
    if (grp == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wave][r][c * 8 + i] = o[r][i];
      if (c == 0) { sm_m[wave][r] = m[r]; sm_l[wave][r] = l[r]; }
    }
  }
  __syncthreads();
  // merge the 4 waves: thread t handles (r, d) pairs
  for (int idx = threadIdx.x; idx < R * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    const int t = TT > 1 ? t0 + r / G : 0, hq = hkv * G + (TT > 1 ? r % G : r);
    if (TT > 1 && t >= p.T) continue;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mm = fmaxf(mm, sm_m[w][r]);
    float ll = 0.f, oo = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float a = mm == -INFINITY ? 0.f : fast_exp2(sm_m[w][r] - mm);
      ll += sm_l[w][r] * a;
      oo += sm_o[w][r][d] * a;
    }
    if constexpr (D == 64) {
      if (p.NS == 1) {  // short cache, one split: this is the whole softmax, no combine launch
        bf16* op = (bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)t * p.o_ts + (int64_t)hq * p.o_hs + d;
        *op = static_cast<bf16>(ll > 0.f ? oo / ll : 0.f);
        continue;
      }
    }
    // partials [B, T, Hq, NS]; one token keeps its 32-bit row index
    const int64_t slot = TT > 1 ? ((int64_t)(b * p.T + t) * p.Hq + hq) * p.NS + split
                                : (int64_t)(b * p.Hq + hkv * G + r) * p.NS + split;
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

template <int D, int G, int TT, typename KT>
void launch_split(const AttnDecodeParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(p.B * p.Hkv), (unsigned)p.NS, (unsigned)((p.T + TT - 1) / TT));
  hipLaunchKernelGGL((attn_decode_split_kernel<D, G, TT, KT>), grid, dim3(256), 0, s, p);
}

template <int D, int G, typename KT>
void launch_tokens(const AttnDecodeParams& p, hipStream_t s) {
  if (p.T == 1) return launch_split<D, G, 1, KT>(p, s);
  if constexpr (G == 8) {
    launch_split<D, 8, 2, KT>(p, s);  // T = 3, 4: two token tiles (see above)
  } else {
    if (p.T == 2) launch_split<D, G, 2, KT>(p, s);
    else if (p.T == 3) launch_split<D, G, 3, KT>(p, s);
    else launch_split<D, G, 4, KT>(p, s);
  }
}

template <int D, typename KT>
void launch_decode(const AttnDecodeParams& p, hipStream_t s) {
  switch (p.Hq / p.Hkv) {
    case 1: launch_tokens<D, 1, KT>(p, s); break;
    case 2: launch_tokens<D, 2, KT>(p, s); break;
    case 4: launch_tokens<D, 4, KT>(p, s); break;
    default: launch_tokens<D, 8, KT>(p, s); break;
  }
  if (D == 64 && p.NS == 1) return;  // the split kernel wrote the output itself
  // the combine kernel sees [B * T] sequences of one token: (b, t) is its batch index (with T = 1
  // the two strides of a contiguous o are the same number)
  AttnDecodeParams c = p;
  c.o_bs = p.o_ts;
  hipLaunchKernelGGL(attn_decode_combine_kernel<D>, dim3((unsigned)(p.B * p.T * p.Hq)), dim3(D), 0, s, c);
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

void attn_decode(const AttnDecodeParams& p, int head_dim, hipStream_t s) {
  if (head_dim == 64) launch_decode<64, bf16>(p, s);
  else launch_decode<128, bf16>(p, s);
}

void attn_decode_fp8(const AttnDecodeParams& p, int head_dim, hipStream_t s) {
  if (head_dim == 64) launch_decode<64, uint8_t>(p, s);
  else launch_decode<128, uint8_t>(p, s);
}

}  // namespace grt
