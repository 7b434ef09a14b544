// fp8 KV cache: the quantising RoPE + cache append of the decode step and the dequantiser.
//
// The cache holds OCP e4m3fn codes [B, L, Hkv, D] (uint8) and one fp32 scale per (token, kv head)
// [B, L, Hkv]; ops/_ref.py::kv_fp8_quantize defines the format and grt_fp8.h holds the encode. The
// split-K decode attention kernel reads the codes directly (decode_attention.hip); the dequantiser
// here serves the chunked-prefill path and the tests.
#include "grt_common.h"
#include "grt_fp8.h"
#include "grt_kernels.h"

namespace grt {
namespace {

constexpr int kNT = 256;

__device__ __forceinline__ uint2 fp8_pack8(const float* x, float scale) {
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i >> 2] |= fp8_quantize(x[i], scale) << (8 * (i & 3));
  return make_uint2(w[0], w[1]);
}

// rope_append_kernel's contract (elementwise.hip) with a quantising cache write: token t (batch row
// t / tpr) at position pos[t]; a position outside the rope table or the cache skips the token (no
// write at all). One lane handles dims [8g, 8g + 8) of both halves of a head, so a head is D / 16
// consecutive lanes (4 or 8: inside one wave, and a wave's loop trip count and the skip predicate
// are the same for all of them); its max |x| is a butterfly over those lanes, which every lane of
// the wave executes. K is rotated in fp32 and rounded to bf16 first: the value the bf16 cache
// would hold is what gets quantised. k_out (optional, bf16 [T, Hkv, D]) receives that value.
__global__ __launch_bounds__(kNT) void rope_append_fp8_kernel(
    const bf16* __restrict__ qkv, int64_t ld, bf16* __restrict__ q_out, bf16* __restrict__ k_out,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc, int64_t c_bs,
    int64_t c_ss, int64_t c_hs, int64_t v_bs, int64_t v_ss, int64_t v_hs, int64_t ks_bs, int64_t ks_ss, int64_t ks_hs,
    int64_t vs_bs, int64_t vs_ss, int64_t vs_hs, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int32_t* __restrict__ pos, int64_t T_, int tpr, int S, int L, int hq, int hkv, int D) {
  const int half = D / 2;
  const int gpp = half / 8;
  const int heads = hq + 2 * hkv;
  const int64_t total = T_ * heads * gpp;
  for (int64_t base = (int64_t)blockIdx.x * kNT; base < total; base += (int64_t)gridDim.x * kNT) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < total;
    const int g = (int)(i % gpp);
    const int64_t th = i / gpp;
    const int h = (int)(th % heads);
    const int64_t t = th / heads;
    const int p = in ? pos[t] : -1;
    const bool ok = in && p >= 0 && p < S && p < L;
    const int64_t b = t / tpr;
    const int c = g * 8;
    float x1[8], x2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x1[k] = x2[k] = 0.f;
    if (ok) {
      const bf16* src = qkv + t * ld + (int64_t)h * D;
      load16(src + c, x1);
      load16(src + half + c, x2);
      if (h < hq + hkv) {
        float cs[8], sn[8];
        load16(cosb + (int64_t)p * half + c, cs); load16(cosb + (int64_t)p * half + c + 4, cs + 4);
        load16(sinb + (int64_t)p * half + c, sn); load16(sinb + (int64_t)p * half + c + 4, sn + 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          // spelled out as the compiler contracts rope_append_kernel's x1 cs - x2 sn / x2 cs + x1 sn:
          // the sin product rounded, the cos product fused, so q and K are bitwise that kernel's
          const float a = fmaf(x1[k], cs[k], -__fmul_rn(x2[k], sn[k]));
          const float r = fmaf(x2[k], cs[k], __fmul_rn(x1[k], sn[k]));
          x1[k] = to_f(static_cast<bf16>(a));
          x2[k] = to_f(static_cast<bf16>(r));
        }
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fmaxf(fabsf(x1[k]), fabsf(x2[k])));
    for (int off = gpp >> 1; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, kWave));
    if (!ok) continue;
    if (h < hq) {
      bf16* dst = q_out + (t * hq + h) * (int64_t)D;
      store16(dst + c, x1);
      store16(dst + half + c, x2);
      continue;
    }
    const bool is_k = h < hq + hkv;
    const int hh = is_k ? h - hq : h - hq - hkv;
    if (is_k && k_out != nullptr) {
      bf16* dst = k_out + (t * hkv + hh) * (int64_t)D;
      store16(dst + c, x1);
      store16(dst + half + c, x2);
    }
    const float scale = fp8_scale(amax);
    uint8_t* dst = is_k ? kc + b * c_bs + (int64_t)p * c_ss + (int64_t)hh * c_hs
                        : vc + b * v_bs + (int64_t)p * v_ss + (int64_t)hh * v_hs;
    *reinterpret_cast<uint2*>(dst + c) = fp8_pack8(x1, scale);
    *reinterpret_cast<uint2*>(dst + half + c) = fp8_pack8(x2, scale);
    if (g == 0) {
      if (is_k) ksc[b * ks_bs + (int64_t)p * ks_ss + (int64_t)hh * ks_hs] = scale;
      else vsc[b * vs_bs + (int64_t)p * vs_ss + (int64_t)hh * vs_hs] = scale;
    }
  }
}

// out[b, j, h, :] = table[codes[b, j, h, :]] * scale[b, j, h] as bf16, j < n; 8 dims per thread
__global__ __launch_bounds__(kNT) void kv_fp8_dequant_kernel(const uint8_t* __restrict__ codes,
                                                             const float* __restrict__ sc, bf16* __restrict__ out,
                                                             int64_t c_bs, int64_t c_ss, int64_t c_hs, int64_t s_bs,
                                                             int64_t s_ss, int64_t s_hs, int64_t B, int n, int H, int D) {
  const int cpr = D / 8;
  const int64_t total = B * n * H * cpr;
  for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kNT) {
    const int c = (int)(i % cpr) * 8;
    int64_t r = i / cpr;
    const int h = (int)(r % H); r /= H;
    const int j = (int)(r % n);
    const int64_t b = r / n;
    const uint2 raw = *reinterpret_cast<const uint2*>(codes + b * c_bs + (int64_t)j * c_ss + (int64_t)h * c_hs + c);
    const float s = sc[b * s_bs + (int64_t)j * s_ss + (int64_t)h * s_hs];
    float f[8];
    fp8x8_to_f32(raw.x, raw.y, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] *= s;
    store16(out + ((b * n + j) * H + h) * (int64_t)D + c, f);
  }
}

inline unsigned grid_for(int64_t work) {
  const int64_t g = (work + kNT - 1) / kNT;
  return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

void rope_append_fp8(const RopeAppendFp8Params& a, hipStream_t s) {
  const int64_t work = a.T * (a.hq + 2 * a.hkv) * (a.D / 16);
  hipLaunchKernelGGL(rope_append_fp8_kernel, dim3(grid_for(work)), dim3(kNT), 0, s, (const bf16*)a.qkv, a.ld,
                     (bf16*)a.q_out, (bf16*)a.k_out, (uint8_t*)a.kc, (uint8_t*)a.vc, a.k_scale, a.v_scale, a.c_bs,
                     a.c_ss, a.c_hs, a.v_bs, a.v_ss, a.v_hs, a.ks_bs, a.ks_ss, a.ks_hs, a.vs_bs, a.vs_ss, a.vs_hs,
                     a.cos, a.sin, a.pos, a.T, a.tpr, a.S, a.L, a.hq, a.hkv, a.D);
}

void kv_fp8_dequant(const void* codes, const float* scale, void* out, int64_t c_bs, int64_t c_ss, int64_t c_hs,
                    int64_t s_bs, int64_t s_ss, int64_t s_hs, int64_t B, int n, int H, int D, hipStream_t s) {
  const int64_t work = B * n * H * (D / 8);
  if (work == 0) return;
  hipLaunchKernelGGL(kv_fp8_dequant_kernel, dim3(grid_for(work)), dim3(kNT), 0, s, (const uint8_t*)codes, scale,
                     (bf16*)out, c_bs, c_ss, c_hs, s_bs, s_ss, s_hs, B, n, H, D);
}

}  // namespace grt
