// Skinny MFMA GEMM for 3-16 decode rows with the decode step's prologues / epilogues: batched
// generate() on a plain bf16 Llama runs the norm-fused step (5 launches per layer) instead of the
// generic one (8-9 launches, a dependent HBM round trip per norm). The contracts are gemv_kernel's
// (gemv.hip), so both kernels can run inside one step on one accumulator workspace.
//
// The weight stream is gemv_mfma_kernel's: 16 weight rows per workgroup, the KS waves split K in
// chunks of 32 kU, kU 16-byte non-temporal loads in flight per lane, every 32-wide K step one
// v_mfma_f32_16x16x32_bf16 (A = the x rows, B = 16 weight rows x 8 consecutive k per lane), the KS
// partial 16x16 tiles merged through LDS. What changes is the A operand and the tail:
//   * PRO_NORMX: lane (c, kg) feeds x row c, so it needs that row's rstd alone: the row's 4 lanes
//     load 16 of its 64 fixed-point slots each and sum them over the kg bits (integer: exact). The
//     slot loads follow the first chunk's weight loads. The fragment is bf16(h * rstd * g).
//   * PRO_SWI: the fragment is bf16(silu(gate) * up) from the fused [M, 2K] gate / up output.
//   * after the LDS merge wave 0 holds column c (one weight row) x rows 4 kg .. 4 kg + 3:
//     EPI_RESNORM writes h = bf16(bf16(y) + res), sums h^2 over the tile's 16 columns with 4
//     xor-shuffles, and lane c = 0 of each kg adds its 4 rows' sums (fixed point) into slot
//     blockIdx.x % 64: one integer atomic per row and workgroup, so the sum stays reproducible;
//     EPI_ROPE: the tile's columns are rows d0 .. d0 + 7 and d0 + HD/2 .. d0 + HD/2 + 7 of one head
//     (d0 = 8 (tile % (HD / 16))), so a RoPE pair is lanes c and c ^ 8: one shuffle per row, then
//     8-lane runs of 16 contiguous bytes into q_out or the cache slot.
// Rows >= M load no x (their A fragments are zero) and write nothing. K % (32 kU) == 0.
// Built without packed fp32 instructions (_build.py KERNEL_FLAGS): the prologue's per-element
// products are what the compiler would pack.
#include "grt_gemv.h"

namespace grt {
namespace {

template <int KS, int PRO, int EPI, int HD>
__global__ __launch_bounds__(64 * KS) void gemv_mfma_fused_kernel(const GemvArgs a, const int M) {
  __shared__ f32x4 red[KS][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = lane & 15, kg = lane >> 4;
  const int N = a.N, K = a.K;
  const int n0 = blockIdx.x * 16;
  const int hh = n0 / HD, d0 = 8 * (blockIdx.x % (HD / 16));  // EPI_ROPE: head and first pair of the tile
  const int n = EPI == EPI_ROPE ? hh * HD + d0 + (c & 7) + (HD / 2) * (c >> 3) : n0 + c;
  const bf16* wr = a.w + (int64_t)min(n, N - 1) * K + kg * 8;
  const bool arow = c < M;
  const bf16* xr = a.x + (int64_t)min(c, M - 1) * a.ldx + kg * 8;
  float rstd = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto chunk = [&](int k, auto first) {
    bf16x8 b[kU], av[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u)
      b[u] = __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wr + k + 32 * u)));
    if constexpr (PRO == PRO_NORMX && decltype(first)::value) {
      unsigned long long v = 0ull;
      if (arow) {
        const unsigned long long* sq = a.sumsq_in + c * kSumsqSlots + kg * (kSumsqSlots / 4);
#pragma unroll
        for (int j = 0; j < kSumsqSlots / 4; ++j) v += sq[j];
      }
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      rstd = rsqrtf(static_cast<float>(v) / kSumsqScale / K + a.eps);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) av[u] = bf16x8{};
    if (arow) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const u32x4 xv = *reinterpret_cast<const u32x4*>(xr + k + 32 * u);
        if constexpr (PRO == PRO_NONE) {
          av[u] = __builtin_bit_cast(bf16x8, xv);
        } else {
          // the other factor: the up half of the [gate | up] row, or the norm weight
          const bf16* op = PRO == PRO_SWI ? xr + K : a.g + kg * 8;
          float xf[8], of[8];
          bf16x8_to_f32(xv, xf);
          bf16x8_to_f32(*reinterpret_cast<const u32x4*>(op + k + 32 * u), of);
#pragma unroll
          for (int j = 0; j < 8; ++j) {  // the roundings of gemv_kernel (the separate kernels' bf16 outputs)
            const float t = PRO == PRO_SWI ? silu_f(xf[j]) * of[j] : xf[j] * rstd * of[j];
            av[u][j] = static_cast<bf16>(t);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[u], b[u], acc, 0, 0, 0);
  };
  int k = wave * 32 * kU;
  if constexpr (PRO == PRO_NORMX) {  // peeled: the statistics are needed by the waves that have work, once
    if (k < K) {
      chunk(k, std::true_type{});
      k += KS * 32 * kU;
    }
  }
  for (; k < K; k += KS * 32 * kU) chunk(k, std::false_type{});
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int q = 1; q < KS; ++q) acc += red[q][lane];
  // D: column c (weight row n), rows 4 kg .. 4 kg + 3
  if constexpr (EPI == EPI_NONE) {
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * kg + r;
        if (m < M) a.y[(int64_t)m * a.ldy + n] = static_cast<bf16>(acc[r]);
      }
    }
  } else if constexpr (EPI == EPI_RESNORM) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * kg + r;
      float s = 0.f;
      if (m < M && n < N) {
        const bf16 yb = static_cast<bf16>(acc[r]);
        const bf16 hb = static_cast<bf16>(static_cast<float>(yb) + static_cast<float>(a.res[(int64_t)m * a.ldr + n]));
        a.y[(int64_t)m * a.ldy + n] = hb;
        const float h = static_cast<float>(hb);
        s = h * h;
      }
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);  // over the 16 columns of this kg
      if (c == 0 && m < M) {
        atomicAdd(a.sumsq_out + m * kSumsqSlots + (blockIdx.x % kSumsqSlots),
                  static_cast<unsigned long long>(llrintf(s * kSumsqScale)));
      }
    }
    if (blockIdx.x == 0) {
      for (int i = lane; i < M * kSumsqSlots; i += 64) a.sumsq_zero[i] = 0ull;
    }
  } else {
    const bool rot = hh < a.hq + a.hkv;  // q and k heads rotate, v heads are copied
    const int d = d0 + (c & 7);
    float yb[4], yo[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // every lane shuffles, before any row is skipped
      yb[r] = static_cast<float>(static_cast<bf16>(acc[r]));  // the bf16 qkv
      yo[r] = __shfl_xor(yb[r], 8, 64);                       // the pair's other half
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * kg + r;
      if (m >= M) continue;
      const int p = a.pos[m];
      if (p < 0 || p >= a.rope_S || p >= a.cache_L) continue;  // like rope_append: no write
      float o = yb[r];
      if (rot) {
        const float cs = a.cosb[(int64_t)p * (HD / 2) + d], sn = a.sinb[(int64_t)p * (HD / 2) + d];
        o = c < 8 ? yb[r] * cs - yo[r] * sn : yb[r] * cs + yo[r] * sn;
      }
      bf16* dst = hh < a.hq         ? a.q_out + ((int64_t)m * a.hq + hh) * HD
                  : hh < a.hq + a.hkv ? a.kc + m * a.c_bs + (int64_t)p * a.c_ss + (int64_t)(hh - a.hq) * a.c_hs
                                      : a.vc + m * a.v_bs + (int64_t)p * a.v_ss + (int64_t)(hh - a.hq - a.hkv) * a.v_hs;
      dst[d + (HD / 2) * (c >> 3)] = static_cast<bf16>(o);
    }
  }
}

template <int PRO, int EPI, int HD = 128>
void launch(const GemvArgs& a, int M, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + 15) / 16));
  // the wave counts of gemv_bf16's MFMA path: 8 while the grid is under ~4 workgroups per CU
  if (a.N <= 16384) hipLaunchKernelGGL((gemv_mfma_fused_kernel<8, PRO, EPI, HD>), grid, dim3(512), 0, s, a, M);
  else hipLaunchKernelGGL((gemv_mfma_fused_kernel<4, PRO, EPI, HD>), grid, dim3(256), 0, s, a, M);
}

}  // namespace

// 3 <= M <= 16, K % 256 == 0 (gemv_mfma_ok), exactly the combinations the decode step uses: a norm
// on load and / or RoPE (qkv, gate_up, lm_head), or the residual epilogue with or without SwiGLU on
// load (down_proj, o_proj)
void gemv_mfma_fused_bf16(const GemvFused& f, hipStream_t s) {
  const GemvArgs a = gemv_args(f);
  const bool normx = f.sumsq_in != nullptr, rope = f.q_out != nullptr;
  const bool d64 = f.head_dim == 64;
  if (rope && normx && d64) launch<PRO_NORMX, EPI_ROPE, 64>(a, f.M, s);
  else if (rope && d64) launch<PRO_NONE, EPI_ROPE, 64>(a, f.M, s);
  else if (rope && normx) launch<PRO_NORMX, EPI_ROPE>(a, f.M, s);
  else if (rope) launch<PRO_NONE, EPI_ROPE>(a, f.M, s);
  else if (normx) launch<PRO_NORMX, EPI_NONE>(a, f.M, s);
  else if (f.swiglu) launch<PRO_SWI, EPI_RESNORM>(a, f.M, s);
  else launch<PRO_NONE, EPI_RESNORM>(a, f.M, s);
}

}  // namespace grt
