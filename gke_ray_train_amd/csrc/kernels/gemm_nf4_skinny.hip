// Skinny MFMA GEMM straight from NF4 codes, with an optional LoRA epilogue, for the 5-16 rows of a
// batched decode step (the binding takes 1-16):
//   y[m][n] = bf16( sum_blocks absmax[n][blk] * sum_{k in blk} x[m][k] * bf16(level[q(n, k)])
//                   + s * sum_r' h[m][i r + r'] * B_i[n - off_i][r'] )               (row n in target i)
//
// Reference role: bitsandbytes' 4-bit inference GEMM under HF ``generate`` on a batch of prompts
// (reference ray-jobs/fine_tune_llama_ray.py:138-146, 215-227). The 1-4-row
// kernel (gemv_nf4.hip) pays a nibble extract, an LDS read and M FMAs per weight and is VALU-bound;
// here the decode is paid once per weight and one v_mfma_f32_16x16x32_bf16 serves up to 16 rows.
//
// Format: what nf4_quantize (nf4.hip) writes — two codes per byte, element 2i in the high nibble,
// blocks of 64 share one fp32 absmax, K % 64 == 0.
//
// Work split: a workgroup owns 16 weight rows, its KS waves (8 from K = 4096, else 4) split K in
// groups of kU quant blocks. Lane (c = lane % 16, kg = lane / 16) holds, per quant block of weight
// row n0 + c, the 16 codes k = 16 kg .. 16 kg + 15 (one 8-byte non-temporal load; four lanes cover
// the block's 32 bytes, kU consecutive blocks the row's 128-byte line) and, as x row c, the same 16
// k of x (rows >= M supply zeros and issue no load). Word 0 of the load feeds the block's first
// MFMA, word 1 the second: the k order inside an MFMA is free as long as A and B agree. Both MFMAs
// go into a zeroed temporary; D puts output column c in every lane, so the block's absmax is one
// scalar per lane and acc = fma(absmax, tmp, acc): no absmax touches a weight, fp32 throughout.
// The next group's codes, absmax and x are loaded before the current group is consumed.
// Decode: the 16 levels, rounded to bf16 (RNE), sit in LDS replicated over the 32 banks ([16][32]
// 32-bit slots, the bf16 in the low half, written by every launch); lane l reads column l % 32, so
// the read is conflict-free for any codes. Per weight: shift, and-or (address), ds_read_b32 and
// half a shift-or (pack) — independent of M.
// Merge: the KS partial tiles go through LDS and wave 0 adds them in wave order: no atomics,
// bitwise reproducible.
// LoRA epilogue (wave 0, issued before the merge barrier): for each target that the tile touches,
// r / 32 (rounded up) more MFMAs into a second accumulator: A = h rows, columns of that target;
// B = the lane's own lora_B row, 8 r' per lane; lanes of another target, of bare rows or past r
// supply zeros. A column belongs to one target, every other target adds exact zeros to it, so the
// order of the target list does not change a bit. Then acc += s * acc_lora.
#include "grt_common.h"
#include "grt_kernels.h"
#include "grt_nf4_table.h"

namespace grt {
namespace {

using nf4_table::decode8;

constexpr int kU = 4;  // quant blocks per lane and K step: 4 x 8 B of codes in flight, twice (prefetch)

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct SkinnyArgs {
  const bf16* x;
  int64_t ldx;
  const uint8_t* q;
  const float* absmax;
  bf16* y;
  int M, N, K;
  // LoRA epilogue
  const bf16* h;  // [M, r * targets], row stride ldh
  int64_t ldh;
  int r, targets;
  float scaling;
  const bf16* b[kNf4GemvMaxTargets];  // lora_B [n_i, r] contiguous
  int off[kNf4GemvMaxTargets], n[kNf4GemvMaxTargets];
};

struct Step {  // one K step of a lane: kU quant blocks
  u32x2 q[kU];
  float am[kU];
  bf16x8 x[kU][2];
};

template <int KS, bool LORA>
__global__ __launch_bounds__(64 * KS) void gemm_nf4_skinny_kernel(const SkinnyArgs a) {
  __shared__ __attribute__((aligned(2048))) uint32_t tab[16 * 32];
  __shared__ f32x4 red[KS][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = lane & 15, kg = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int M = a.M, N = a.N, K = a.K;
  const int row = min(n0 + c, N - 1);  // rows past N read row N - 1, never stored
  const uint8_t* __restrict__ qr = a.q + (((int64_t)row * K) >> 1) + kg * 8;
  const float* __restrict__ ar = a.absmax + (int64_t)row * (K >> 6);
  const bool arow = c < M;
  const bf16* __restrict__ xr = a.x + (int64_t)min(c, M - 1) * a.ldx + kg * 16;
  // blocks past K (the last step of a wave) load nothing and contribute 0 * 0
  auto load = [&](int k, Step& s) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int kb = k + 64 * u;
      s.q[u] = u32x2{0u, 0u}, s.am[u] = 0.f, s.x[u][0] = bf16x8{}, s.x[u][1] = bf16x8{};
      if (kb < K) {
        s.q[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(qr + (kb >> 1)));
        s.am[u] = __builtin_nontemporal_load(ar + (kb >> 6));
        if (arow) {
          s.x[u][0] = *reinterpret_cast<const bf16x8*>(xr + kb);
          s.x[u][1] = *reinterpret_cast<const bf16x8*>(xr + kb + 8);
        }
      }
    }
  };
  // the first step's loads are issued before the table is built: its constant loads, LDS writes and
  // barrier sit under the HBM latency
  Step cur, nxt;
  int k = wave * 64 * kU;
  if (k < K) load(k, cur);
  nf4_table::fill<64 * KS>(tab);
  __syncthreads();
  const uint32_t col = nf4_table::column(tab, lane);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  while (k < K) {
    const int kn = k + KS * 64 * kU;
    if (kn < K) load(kn, nxt);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.x[u][0], decode8(cur.q[u][0], col), t, 0, 0, 0);
      t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.x[u][1], decode8(cur.q[u][1], col), t, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = fmaf(cur.am[u], t[r], acc[r]);
    }
    cur = nxt;
    k = kn;
  }
  f32x4 accl = {0.f, 0.f, 0.f, 0.f};
  if constexpr (LORA) {
    if (wave == 0) {
      const int n = n0 + c, r = a.r;
      // constant indices into the by-value arguments (scalar selects; gemv_nf4.hip)
#pragma unroll
      for (int i = 0; i < kNf4GemvMaxTargets; ++i) {
        if (i < a.targets && n0 < a.off[i] + a.n[i] && n0 + 16 > a.off[i]) {  // the tile touches target i
          const bool mine = n >= a.off[i] && n < a.off[i] + a.n[i];
          const bf16* bp = a.b[i] + (int64_t)(n - a.off[i]) * r;
          const bf16* hp = a.h + (int64_t)c * a.ldh + i * r;
          for (int k0 = 0; k0 < r; k0 += 32) {
            const int kk = k0 + kg * 8;  // r % 8 == 0: a lane's 8 r' are all inside r or all past it
            bf16x8 av = bf16x8{}, bv = bf16x8{};
            if (arow && kk < r) av = *reinterpret_cast<const bf16x8*>(hp + kk);
            if (mine && kk < r) bv = *reinterpret_cast<const bf16x8*>(bp + kk);
            accl = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, accl, 0, 0, 0);
          }
        }
      }
    }
  }
  if (wave != 0) red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 1; w < KS; ++w) {
    const f32x4 p = red[w][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += p[r];
  }
  const int n = n0 + c;  // D: column c, rows 4 kg .. 4 kg + 3
  if (n < N) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * kg + r;
      if (m < M) a.y[(int64_t)m * N + n] = static_cast<bf16>(LORA ? fmaf(a.scaling, accl[r], acc[r]) : acc[r]);
    }
  }
}

template <bool LORA>
void launch_skinny(const SkinnyArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 15) / 16));
  // one K step of a wave is kU blocks = 256 elements: 8 waves from a Llama-size row (2+ steps each)
  if (a.K >= 4096) hipLaunchKernelGGL((gemm_nf4_skinny_kernel<8, LORA>), grid, dim3(512), 0, s, a);
  else hipLaunchKernelGGL((gemm_nf4_skinny_kernel<4, LORA>), grid, dim3(256), 0, s, a);
}

}  // namespace

void gemm_nf4_skinny(const Nf4GemmSkinny& f, hipStream_t s) {
  SkinnyArgs a{};
  a.x = static_cast<const bf16*>(f.x), a.ldx = f.ldx, a.q = f.q, a.absmax = f.absmax;
  a.y = static_cast<bf16*>(f.y), a.M = f.M, a.N = f.N, a.K = f.K;
  a.h = static_cast<const bf16*>(f.h), a.ldh = f.ldh, a.r = f.r, a.targets = f.targets, a.scaling = f.scaling;
  for (int i = 0; i < f.targets; ++i) a.b[i] = static_cast<const bf16*>(f.b[i]), a.off[i] = f.off[i], a.n[i] = f.n[i];
  if (f.targets > 0) launch_skinny<true>(a, s);
  else launch_skinny<false>(a, s);
}

}  // namespace grt
