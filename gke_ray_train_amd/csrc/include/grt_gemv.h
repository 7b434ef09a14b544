// What the decode GEMV kernels share (gemv.hip: the FMA GEMV and the plain MFMA skinny GEMM;
// gemv_mfma_fused.hip: the MFMA skinny GEMM with the step's prologues / epilogues): the prologue /
// epilogue selectors, the fixed-point accumulator layout and the kernel argument block. The
// contracts are documented at the head of gemv.hip.
#pragma once
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

__device__ __forceinline__ float silu_f(float g) { return g / (1.f + __expf(-g)); }

// input transform of x
enum { PRO_NONE = 0, PRO_SWI = 1, PRO_NORMX = 2 };
// output
enum { EPI_NONE = 0, EPI_RESNORM = 1, EPI_ROPE = 2 };

constexpr float kSumsqScale = 1048576.f;  // 2^20: fixed-point units of the sum-of-squares accumulator
constexpr int kSumsqSlots = 64;           // accumulator addresses per row: workgroup b adds into b % 64

constexpr int kU = 8;  // MFMA skinny kernels: 32-wide K steps per wave per iteration

struct GemvArgs {
  const bf16* x;
  int64_t ldx;
  const bf16* w;
  bf16* y;  // EPI_RESNORM: h = y + res
  int64_t ldy;
  int N, K;
  const bf16* g;  // PRO_NORMX: norm weight [K]
  float eps;      // PRO_NORMX
  const unsigned long long* sumsq_in;  // PRO_NORMX: [M][kSumsqSlots] fixed-point partial sums of h^2
  // EPI_RESNORM
  const bf16* res;  // [M, N], row stride ldr
  int64_t ldr;
  unsigned long long* sumsq_out;   // [M][kSumsqSlots], zero at launch
  unsigned long long* sumsq_zero;  // [M][kSumsqSlots], zeroed here for the next producer
  // EPI_ROPE (the qkv projection, head_dim HD = 128 or 64): q rotated into q_out [M, hq, HD], k
  // rotated and v written at cache slot pos[m] of kc / vc (row m = batch row m)
  bf16* q_out;
  bf16* kc;
  bf16* vc;
  int64_t c_bs, c_ss, c_hs, v_bs, v_ss, v_hs;
  const float* cosb;  // [>= rope_S, HD / 2]
  const float* sinb;
  const int* pos;     // [M]
  int rope_S, cache_L, hq, hkv;
};

inline GemvArgs gemv_args(const GemvFused& f) {
  GemvArgs a{};
  a.x = static_cast<const bf16*>(f.x), a.ldx = f.ldx, a.w = static_cast<const bf16*>(f.w);
  a.y = static_cast<bf16*>(f.y), a.ldy = f.ldy, a.N = f.N, a.K = f.K;
  a.g = static_cast<const bf16*>(f.g), a.eps = f.eps, a.sumsq_in = f.sumsq_in;
  a.res = static_cast<const bf16*>(f.res), a.ldr = f.ldr, a.sumsq_out = f.sumsq_out, a.sumsq_zero = f.sumsq_zero;
  a.q_out = static_cast<bf16*>(f.q_out), a.kc = static_cast<bf16*>(f.kc), a.vc = static_cast<bf16*>(f.vc);
  a.c_bs = f.c_bs, a.c_ss = f.c_ss, a.c_hs = f.c_hs, a.v_bs = f.v_bs, a.v_ss = f.v_ss, a.v_hs = f.v_hs;
  a.cosb = f.cosb, a.sinb = f.sinb, a.pos = f.pos, a.rope_S = f.rope_S, a.cache_L = f.cache_L;
  a.hq = f.hq, a.hkv = f.hkv;
  return a;
}

}  // namespace
}  // namespace grt
