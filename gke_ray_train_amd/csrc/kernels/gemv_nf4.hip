// Decode GEMV straight from NF4 codes, with an optional LoRA epilogue:
//   y[m][n] = bf16( sum_k x[m][k] * code[q(n, k)] * absmax[(n K + k) / 64]
//                   + s * sum_r' h[m][j r + r'] * B_i[n - off_i][r'] )      (row n in target i)
//
// Reference role: bitsandbytes' 4-bit inference GEMV under HF ``generate`` on a QLoRA model
// (reference ray-jobs/fine_tune_llama_ray.py:138-146, 215-227). The training
// path dequantises a projection into bf16 and runs the library GEMM; for the 1-4 rows of a decode
// step that writes and re-reads 2 B/param where the step needs the 0.5 B/param of codes once.
//
// Format: what nf4_quantize (nf4.hip) writes — two codes per byte, element 2i in the high nibble,
// blocks of 64 share one fp32 absmax, K % 64 == 0 (a block never straddles a row, rows start
// 16-byte aligned). The weight is the exact NF4 value, fp32 code-book level times fp32 absmax (not
// the bf16-rounded weight of the dequantisers), so the absmax is factored out of a lane's partial
// sum: a 16-byte non-temporal load is 32 codes, half a quant block, one absmax.
//
// Structure (gemv.hip's): each wave owns kR = 4 weight rows, KS waves of the workgroup split K and
// merge through LDS, x (M x K bf16, a few KB) is re-read from cache, fp32 accumulation, one wave
// butterfly per (m, row), no atomics: bitwise reproducible. KS follows K (4 from 8192, 2 from 4096,
// else 1) so that a Llama-size row keeps every lane loading; smaller K leaves lanes idle.
// Lookup: the 16 levels sit in LDS replicated over the 32 banks ([16][32] floats, 2 KiB, written by
// every launch), lane l reads column l % 32: ds_read_b32, conflict-free for any codes. Per weight:
// a nibble extract, an address, one LDS read and M FMAs.
// LoRA epilogue: lanes r' < r of the wave that holds the final sums add s * h[m][j r + r'] *
// B_i[n - off_i][r'] (loaded ahead of the K loop) into their accumulators before the butterfly (no
// extra reduction, no block-diagonal B buffer). off_i % 4 == 0, so a wave's rows start in one target; each row looks
// its target up on its own (n_i need not be a multiple of 4).
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

constexpr int kR = 4;  // weight rows per wave

__constant__ float kLevels[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

struct Nf4GemvArgs {
  const bf16* x;
  int64_t ldx;
  const uint8_t* q;
  const float* absmax;
  bf16* y;
  int N, K;
  // LoRA epilogue
  const bf16* h;  // [M, r * targets], row stride ldh
  int64_t ldh;
  int r, targets;
  float scaling;
  const bf16* b[kNf4GemvMaxTargets];  // lora_B [n_i, r] contiguous
  int off[kNf4GemvMaxTargets], n[kNf4GemvMaxTargets];
};

template <int M, int KS, bool LORA>
__global__ __launch_bounds__(256) void gemv_nf4_kernel(const Nf4GemvArgs a) {
  __shared__ float tab[16 * 32];
  __shared__ float red[4][M][kR];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = wave / KS, kp = wave % KS;
  const int n0 = (blockIdx.x * (4 / KS) + slot) * kR;
  const int N = a.N, K = a.K;
  const float* __restrict__ tl = tab + (lane & 31);
  const bf16* __restrict__ x = a.x;
  float acc[M][kR];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[m][r] = 0.f;
  int64_t rowbase[kR];  // first element of the row (rows past N read row N - 1, never stored)
#pragma unroll
  for (int r = 0; r < kR; ++r) rowbase[r] = (int64_t)min(n0 + r, N - 1) * K;
  // the first K-step's weight loads are issued before the table is built (the table's constant
  // loads, LDS writes and barrier then sit under the HBM latency), and every later step's before
  // the current one is consumed
  u32x4 nv[kR];
  float na[kR];
  auto load = [&](int k) {
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      nv[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.q + ((rowbase[r] + k) >> 1)));
      na[r] = __builtin_nontemporal_load(a.absmax + ((rowbase[r] + k) >> 6));
    }
  };
  int k = (kp * 64 + lane) * 32;
  if (k < K) load(k);
  // LoRA operands of lane r' as raw bf16. Every lane of every wave loads from a valid address (a
  // row without a target reads target 0's first row, lanes past r read column r - 1) and on[r]
  // masks the product afterwards: straight-line loads that nothing waits for until the epilogue.
  // The target of a row is picked with constant indices into the by-value arguments (scalar
  // selects); an index computed at run time turns every argument read into a vector load, and
  // with branches around the loads each row becomes a chain of dependent round trips (gate_up
  // +13 us). With 1-2 rows the loads go out here, ahead of the table and the K loop; with 3-4 rows
  // the registers they would hold through the loop cost a wave per SIMD, so they go out after it.
  uint32_t braw[kR], hraw[M][kR];
  bool on[kR];
  auto lora_load = [&]() {
    const int ll = min(lane, a.r - 1);
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int row = n0 + r;
      const bf16* bp = a.b[0];
      int hc = 0;
      bool hit = false;
#pragma unroll
      for (int i = 0; i < kNf4GemvMaxTargets; ++i) {
        if (i < a.targets && row < N && row >= a.off[i] && row < a.off[i] + a.n[i]) {
          bp = a.b[i] + (int64_t)(row - a.off[i]) * a.r;
          hc = i * a.r;
          hit = true;
        }
      }
      on[r] = hit && kp == 0 && lane < a.r;
      braw[r] = reinterpret_cast<const unsigned short*>(bp)[ll];
#pragma unroll
      for (int m = 0; m < M; ++m) hraw[m][r] = reinterpret_cast<const unsigned short*>(a.h)[m * a.ldh + hc + ll];
    }
  };
  constexpr bool kLoraEarly = M <= 2;
  if constexpr (LORA && kLoraEarly) lora_load();
  tab[threadIdx.x] = kLevels[threadIdx.x >> 5];
  tab[256 + threadIdx.x] = kLevels[8 + (threadIdx.x >> 5)];
  __syncthreads();
  while (k < K) {
    u32x4 wv[kR];
    float am[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) wv[r] = nv[r], am[r] = na[r];
    const int kn = k + KS * 64 * 32;
    if (kn < K) load(kn);
    float part[M][kR];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < kR; ++r) part[m][r] = 0.f;
#pragma unroll
    for (int wi = 0; wi < 4; ++wi) {  // word wi = elements k + 8 wi .. + 7
      float xf[M][8];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const u32x4 xv = *reinterpret_cast<const u32x4*>(x + m * a.ldx + k + 8 * wi);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xf[m][2 * i] = __uint_as_float(xv[i] << 16);
          xf[m][2 * i + 1] = __uint_as_float(xv[i] & 0xffff0000u);
        }
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const uint32_t w = wv[r][wi];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // byte j: element 2j in its high nibble, 2j + 1 in its low
          const float hi = tl[((w >> (8 * j + 4)) & 15u) * 32];
          const float lo = tl[((w >> (8 * j)) & 15u) * 32];
#pragma unroll
          for (int m = 0; m < M; ++m) {
            part[m][r] = fmaf(xf[m][2 * j], hi, part[m][r]);
            part[m][r] = fmaf(xf[m][2 * j + 1], lo, part[m][r]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < kR; ++r) acc[m][r] = fmaf(am[r], part[m][r], acc[m][r]);
    k = kn;
  }
  if constexpr (LORA) {
    if constexpr (!kLoraEarly) lora_load();
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < kR; ++r)
        acc[m][r] = fmaf(a.scaling * __uint_as_float(hraw[m][r] << 16), on[r] ? __uint_as_float(braw[r] << 16) : 0.f,
                         acc[m][r]);
  }
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      float v = acc[m][r];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      acc[m][r] = v;
    }
  if constexpr (KS > 1) {
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int r = 0; r < kR; ++r) red[wave][m][r] = acc[m][r];
    }
    __syncthreads();
    if (kp == 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int r = 0; r < kR; ++r) {
          float v = 0.f;
#pragma unroll
          for (int q = 0; q < KS; ++q) v += red[slot * KS + q][m][r];
          acc[m][r] = v;
        }
    }
  }
  if (lane == 0 && kp == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < kR; ++r)
        if (n0 + r < N) a.y[(int64_t)m * N + n0 + r] = static_cast<bf16>(acc[m][r]);
  }
}

template <int KS, bool LORA>
void launch_ks(const Nf4GemvArgs& a, int M, hipStream_t s) {
  const int rows_per_wg = (4 / KS) * kR;
  const dim3 grid((unsigned)((a.N + rows_per_wg - 1) / rows_per_wg));
  switch (M) {
    case 1: hipLaunchKernelGGL((gemv_nf4_kernel<1, KS, LORA>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((gemv_nf4_kernel<2, KS, LORA>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((gemv_nf4_kernel<3, KS, LORA>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((gemv_nf4_kernel<4, KS, LORA>), grid, dim3(256), 0, s, a); break;
  }
}

template <bool LORA>
void launch_nf4(const Nf4GemvArgs& a, int M, hipStream_t s) {
  // one K-step of a wave is 64 lanes x 32 codes = 2048 elements
  if (a.K >= 8192) launch_ks<4, LORA>(a, M, s);
  else if (a.K >= 4096) launch_ks<2, LORA>(a, M, s);
  else launch_ks<1, LORA>(a, M, s);
}

}  // namespace

void gemv_nf4(const Nf4Gemv& f, hipStream_t s) {
  Nf4GemvArgs a{};
  a.x = static_cast<const bf16*>(f.x), a.ldx = f.ldx, a.q = f.q, a.absmax = f.absmax;
  a.y = static_cast<bf16*>(f.y), a.N = f.N, a.K = f.K;
  a.h = static_cast<const bf16*>(f.h), a.ldh = f.ldh, a.r = f.r, a.targets = f.targets, a.scaling = f.scaling;
  for (int i = 0; i < f.targets; ++i) a.b[i] = static_cast<const bf16*>(f.b[i]), a.off[i] = f.off[i], a.n[i] = f.n[i];
  if (f.targets > 0) launch_nf4<true>(a, f.M, s);
  else launch_nf4<false>(a, f.M, s);
}

}  // namespace grt
