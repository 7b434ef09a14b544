// LoRA training kernels for ranks 8, 16 and 32 on gfx950 / CDNA4: the one-pass products of lora.hip
// and lora_grad.hip (built for the reference config's r = 64) on 16-wide rank tiles.
//
// Reference role: PEFT's LoRA layer and its backward on every adapted projection of the QLoRA SFT job
// (reference ray-jobs/fine_tune_llama_ray.py:243-254; LORA_R of fine_tune_config.json:6-8 is a user
// key, PEFT's default rank is 8). Per adapted module, R = r * targets (<= 96):
//     h'   = s drop(x) A_cat^T    [M, R]     down   (lora_small_nt, one product, dropout on A's side)
//     g_i  = s dY_i B_i           [M, r]     g      (lora_small_nt, up to 4 products)
//     dB_i = dY_i^T h'_i          [n_i, r]   tred, plain output
//     dA   = g^T x_d              [R, in]    tred, transposed output
//     dX  += keep/(1-p) (g A)     [M, in]    dx     (R = 8 / 24; lora_dx takes R % 16 == 0)
// and the refresh of the B blocks in the tail of W' and in the B^T buffer.
//
// Rank tile: v_mfma_f32_16x16x32_bf16 (as gemm_nf4_skinny.hip). The 32x32x16 tiles of the r = 64
// kernels would spend half (r = 16) or three quarters (r = 8) of every MFMA on padding. r = 8 and the
// odd multiples of 8 are padded to 16 in the LDS image only: operands and outputs keep their true
// r-wide rows (r % 8 == 0: 16-byte rows, strides % 8 == 0). Where the rank is an OUTPUT index (nt,
// tred) the pad rows / columns of the image repeat a valid row / chunk and the accumulator rows they
// produce are never stored; where it is the REDUCTION index (dx) the pad is zero in the fragment
// registers.
//
// Work split: the big [tokens, features] operand is read once, by LDS-DMA into the swizzled image
// (grt_lds_image.h) through a 4-slot ring with a counted vmcnt across raw s_barriers (lora_grad.hip's
// pipeline).
//   nt    One workgroup = 32 tokens x all of K (or one k range of a split). The small operand B^T
//         [r][K] is at most 48 x 14336 bf16 = 1.3 MiB: it cannot stay in LDS, so its [16 RT][128]
//         tile is re-streamed through the same ring (4-12 KiB against the 8 KiB token tile; it stays
//         in L2, every workgroup reads the same rows). Wave w owns token tile w & 1 and the k-steps
//         2 (w >> 1), + 1 of each tile; D[rank][token] gives a lane 4 consecutive ranks of one token,
//         an 8-byte store. The two k halves are summed through LDS; k splits (few row blocks) leave
//         fp32 partials for lora_small_nt_fin, summed in index order.
//   tred  One workgroup = 128 columns of A x one token range, 32-token tiles. H [M][R <= 96] fits one
//         128-column image per tile and is needed by every wave, so it rides in the ring next to A
//         (re-streamed per column block from L2; it is R / N of A's bytes). Both feed the MFMAs by
//         transposed reads (ds_read_b64_tr_b16): one MFMA reduces the whole 32-token tile. The last
//         tile of a range may be partial: its DMA rows are clamped to M - 1 and the H fragment is
//         zeroed past the range. fp32 partials per token range in the output layout, then
//         lora_small_tred_fin: index-ordered, no atomics.
//   dx    g [M][R] and A^T [K][R] are dense and tiny (16-48 bytes per row, contiguous): fragments come
//         straight from global / L2 with zero fill past R, nothing is staged. One workgroup = 64
//         tokens x 128 columns of dX; the fp32 tile goes through LDS so dX moves in 16-byte pieces of
//         full rows, with lora_dx's mask / scale / add epilogue.
#include "grt_common.h"
#include "grt_kernels.h"
#include "grt_lds_image.h"

namespace grt {
namespace {

using namespace lds_image;

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// A: lane (i = lane & 15, kg = lane >> 4) holds A[i][8 kg .. 8 kg + 7]; B: B[8 kg ..][j = lane & 15];
// D: lane holds D[4 kg .. 4 kg + 3][lane & 15].

template <class T>
__device__ __forceinline__ T pick(const T (&v)[4], int t) {
  return t == 0 ? v[0] : t == 1 ? v[1] : t == 2 ? v[2] : v[3];
}

// lora.hip's element-dropout mask of 8 consecutive elements from a 4-aligned element index
__device__ __forceinline__ void keep8(uint64_t key, uint64_t idx0, uint32_t thr, bool (&kp)[8]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint64_t hv = hash_u64(key ^ ((idx0 >> 2) + q));
#pragma unroll
    for (int j = 0; j < 4; ++j) kp[4 * q + j] = ((uint32_t)(hv >> (16 * j)) & 0xffffu) >= thr;
  }
}

constexpr int NS = 4;            // ring slots
constexpr int IMG = 32 * 256;    // one 32-row x 128-column image: 8 KiB

// wait until at most nd tiles' DMAs (D instructions each) and ns store groups (S each) issued after
// the wanted tile are still in flight; nd, ns in 0 .. 2
template <int D, int S>
__device__ __forceinline__ void wait_tile(int nd, int ns) {
  switch (nd * 3 + ns) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(S) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * S) : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(D) : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(D + S) : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(D + 2 * S) : "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * D) : "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * D + S) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * D + 2 * S) : "memory"); break;
  }
}

// ---------------------------------------------------------------------------------------------
// nt: C[M][r] (+)= alpha A[M][K] B^T[r][K]^T
// ---------------------------------------------------------------------------------------------
template <int RT, bool DROP, bool XD>  // r <= 16 RT
__global__ __launch_bounds__(256) void nt_kernel(const LoraSmallNtParams P) {
  constexpr int SLOT = IMG + 16 * RT * 256;
  constexpr int D = 2 + RT;       // DMA instructions per wave and tile
  constexpr int S = XD ? 2 : 0;   // x_d stores per wave and tile
  __shared__ __attribute__((aligned(16))) char smem[NS * SLOT];
  const int tid = threadIdx.x, lane = tid & 63, kg = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tt = w & 1, ksl = w >> 1;
  const int pt = blockIdx.y;
  const int nrb = (int)((P.M + 31) / 32);
  const int rb = blockIdx.x % nrb, ksi = blockIdx.x / nrb;
  const int64_t m0 = (int64_t)rb * 32;
  const int K = pick(P.K, pt);
  const int64_t lda = pick(P.lda, pt), ldbt = pick(P.ldbt, pt), ldc = pick(P.ldc, pt);
  const int nkt_all = K / 128;
  const int kt0 = ksi * nkt_all / P.ks;
  const int nt = (ksi + 1) * nkt_all / P.ks - kt0;
  const bf16* A = static_cast<const bf16*>(pick(P.a, pt));
  const bf16* BT = static_cast<const bf16*>(pick(P.bt, pt));
  // DMA sources: wave w fills A rows 8w .. 8w + 7 (2 pieces of 4 rows) and B^T image rows
  // 4 RT w .. (RT pieces); rows past M / past r repeat the last valid row (never stored)
  const bf16* asrc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = 8 * w + 4 * q + kg;
    const int64_t m = min(m0 + r, P.M - 1);
    asrc[q] = A + m * lda + (int64_t)kt0 * 128 + 8 * (l16 ^ swz(r));
  }
  const bf16* bsrc[RT];
#pragma unroll
  for (int q = 0; q < RT; ++q) {
    const int r = 4 * RT * w + 4 * q + kg;
    bsrc[q] = BT + (int64_t)min(r, P.r - 1) * ldbt + (int64_t)kt0 * 128 + 8 * (l16 ^ swz(r));
  }
  const uint32_t smem0 = lds_addr(smem);
  auto dma_tile = [&](int t, int slot) __attribute__((always_inline)) {
    const uint32_t base = smem0 + (uint32_t)(slot * SLOT);
    const uint32_t da = __builtin_amdgcn_readfirstlane(base + (uint32_t)(8 * w * 256));
    const uint32_t db = __builtin_amdgcn_readfirstlane(base + (uint32_t)(IMG + 4 * RT * w * 256));
#pragma unroll
    for (int q = 0; q < 2; ++q) lds_dma16(asrc[q] + t * 128, da + q * 1024);
#pragma unroll
    for (int q = 0; q < RT; ++q) lds_dma16(bsrc[q] + t * 128, db + q * 1024);
  };
  const uint32_t thr = drop_thr(P.p);
  const float sc = DROP ? 1.f / (1.f - P.p) : 1.f;
  const uint64_t key = hash_u64(P.seed);
  const int64_t mytok = m0 + 16 * tt + l16;
  // a lane past the last token holds row M - 1 (clamped DMA source) and stores what that row's own
  // lane stores: every wave issues the same number of x_d stores, which the counted vmcnt relies on
  const int64_t tokc = min(mytok, P.M - 1);
  bf16* xdrow = XD ? static_cast<bf16*>(P.xd) + tokc * (int64_t)K + (int64_t)kt0 * 128 : nullptr;
  const uint64_t eidx0 = P.offset + (uint64_t)tokc * (uint64_t)K + (uint64_t)kt0 * 128;

  f32x4 acc[RT];
#pragma unroll
  for (int j = 0; j < RT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int pre = min(nt, NS - 1);
  for (int t = 0; t < pre; ++t) dma_tile(t, t);
  for (int t = 0; t < nt; ++t) {
    const int slot = t % NS;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of slot t-1 are done
    wait_tile<D, S>(min(2, nt - 1 - t), min(t, 2));      // tile t landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                         // ... every wave's; slot t-1 free
    const char* ai = smem + slot * SLOT;
    const char* bi = ai + IMG;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int ch = 4 * (2 * ksl + s2) + kg;  // 16-byte chunk of this lane's 8 k
      bf16x8 xf = *reinterpret_cast<const bf16x8*>(ai + chunk_off(16 * tt + l16, ch));
      if (DROP) {
        bool kp[8];
        keep8(key, eidx0 + (uint64_t)t * 128 + 8 * ch, thr, kp);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[e] = static_cast<bf16>(kp[e] ? static_cast<float>(xf[e]) * sc : 0.f);
      }
      if (XD) *reinterpret_cast<bf16x8*>(xdrow + t * 128 + 8 * ch) = xf;
#pragma unroll
      for (int j = 0; j < RT; ++j)
        acc[j] = mfma16(*reinterpret_cast<const bf16x8*>(bi + chunk_off(16 * j + l16, ch)), xf, acc[j]);  // D[rank][token]
    }
    if (t + NS - 1 < nt) dma_tile(t + NS - 1, (t + NS - 1) % NS);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // ring consumed: the space takes the k-half reduction
  f32x4* red = reinterpret_cast<f32x4*>(smem);  // [2 token tiles][RT][64 lanes]
  if (ksl > 0) {
#pragma unroll
    for (int j = 0; j < RT; ++j) red[(tt * RT + j) * 64 + lane] = acc[j];
  }
  __syncthreads();
  if (ksl > 0 || mytok >= P.M) return;
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int rr = 16 * j + 4 * kg;  // this lane's 4 ranks: all inside r or all past it (r % 4 == 0)
    if (rr >= P.r) continue;
    const f32x4 v = acc[j] + red[(tt * RT + j) * 64 + lane];
    if (P.ks > 1) {  // fp32 partial of this k range; nt_fin_kernel sums them
      *reinterpret_cast<f32x4*>(P.ws + (((int64_t)pt * P.ks + ksi) * P.M + mytok) * P.r + rr) = v;
      continue;
    }
    bf16x4* dst = reinterpret_cast<bf16x4*>(static_cast<bf16*>(pick(P.c, pt)) + mytok * ldc + rr);
    const bf16x4 old = P.accumulate ? *dst : bf16x4{};
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = static_cast<bf16>(P.alpha * v[e] + (P.accumulate ? static_cast<float>(old[e]) : 0.f));
    *dst = o;
  }
}

// C[m][0 .. r) (+)= alpha * sum_k ws[k][m][..] (grid y = product)
__global__ __launch_bounds__(256) void nt_fin_kernel(const LoraSmallNtParams P) {
  const int pt = blockIdx.y, r4 = P.r / 4;
  const int64_t n4 = P.M * r4, plane = P.M * P.r;
  bf16* C = static_cast<bf16*>(pick(P.c, pt));
  const int64_t ldc = pick(P.ldc, pt);
  const float* ws = P.ws + (int64_t)pt * P.ks * plane;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / r4, c = (e % r4) * 4;
    f32x4 s = *reinterpret_cast<const f32x4*>(ws + 4 * e);
    for (int k = 1; k < P.ks; ++k) s += *reinterpret_cast<const f32x4*>(ws + k * plane + 4 * e);
    bf16x4* dst = reinterpret_cast<bf16x4*>(C + m * ldc + c);
    const bf16x4 old = P.accumulate ? *dst : bf16x4{};
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = static_cast<bf16>(P.alpha * s[q] + (P.accumulate ? static_cast<float>(old[q]) : 0.f));
    *dst = o;
  }
}

// ---------------------------------------------------------------------------------------------
// tred: out = alpha A^T H
// ---------------------------------------------------------------------------------------------
template <int JT>  // R <= 16 JT
__global__ __launch_bounds__(256) void tred_kernel(const LoraTredParams P) {
  constexpr int SLOT = 2 * IMG;    // A image + H image
  constexpr int TS = 16 * JT + 4;  // fp32 output tile row
  static_assert(128 * TS * 4 <= NS * SLOT, "the output tile reuses the ring");
  __shared__ __attribute__((aligned(16))) char smem[NS * SLOT];
  const int tid = threadIdx.x, lane = tid & 63, kg = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = P.R;
  const int gb = blockIdx.x % P.nbt, ks = blockIdx.x / P.nbt;  // column block of the launch, split
  const int pt = (gb >= P.bo[1]) + (gb >= P.bo[2]) + (gb >= P.bo[3]);  // product (bo past nprod: INT_MAX)
  const int nb = gb - pick(P.bo, pt);
  const int N = pick(P.N, pt);
  const int64_t lda = pick(P.lda, pt), ldh = pick(P.ldh, pt);
  const int64_t mbeg = (int64_t)ks * P.mchunk;
  const int64_t mend = min(P.M, mbeg + P.mchunk);
  const int nt = mend > mbeg ? (int)((mend - mbeg + 31) / 32) : 0;
  const bf16* A = static_cast<const bf16*>(pick(P.a, pt)) + (int64_t)nb * 128;
  const bf16* H = static_cast<const bf16*>(pick(P.h, pt));

  // LDS-DMA of tile t: wave w fills image rows 8w .. 8w + 7 (two 1-KiB pieces of 4 rows) of the A and
  // of the H image; the XOR swizzle is applied to the per-lane SOURCE chunk. Rows past M repeat row
  // M - 1 (masked below); H chunks past column R repeat a valid chunk (their outputs are not stored).
  const uint32_t smem0 = lds_addr(smem);
  const int row0 = 8 * w + kg, row1 = row0 + 4;
  const int ch0 = l16 ^ swz(row0), ch1 = l16 ^ swz(row1);
  const int hc0 = ch0 % (R / 8), hc1 = ch1 % (R / 8);
  auto dma_tile = [&](int t, int slot) __attribute__((always_inline)) {
    const int64_t r0 = min(mbeg + 32 * t + row0, P.M - 1), r1 = min(mbeg + 32 * t + row1, P.M - 1);
    const uint32_t dst = __builtin_amdgcn_readfirstlane(smem0 + (uint32_t)(slot * SLOT + 8 * w * 256));
    lds_dma16(A + r0 * lda + 8 * ch0, dst);
    lds_dma16(A + r1 * lda + 8 * ch1, dst + 1024);
    lds_dma16(H + r0 * ldh + 8 * hc0, dst + IMG);
    lds_dma16(H + r1 * ldh + 8 * hc1, dst + IMG + 1024);
  };

  f32x4 acc[2][JT];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[n][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int pre = min(nt, NS - 1);
  for (int t = 0; t < pre; ++t) dma_tile(t, t);
  for (int t = 0; t < nt; ++t) {
    const int slot = t % NS;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of slot t-1 are done
    wait_tile<4, 0>(min(2, nt - 1 - t), 0);             // tile t landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();                        // ... every wave's; slot t-1 free
    if (t + NS - 1 < nt) dma_tile(t + NS - 1, (t + NS - 1) % NS);
    const char* ai = smem + slot * SLOT;
    const char* hi = ai + IMG;
    // the MFMA's 32 k are the tile's tokens: lane group kg holds tokens 4 kg .. + 3 and 16 + 4 kg .. + 3
    // (the two row quads of a 32-lane half then differ in (row >> 2) & 3: no bank conflict)
    const int rem = (int)min((int64_t)32, mend - (mbeg + 32 * t));  // valid tokens of this tile (wave-uniform)
    bf16x8 a[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c0 = 32 * w + 16 * n;
      a[n] = cat(tr_read(ai, 4 * kg, c0, l16), tr_read(ai, 16 + 4 * kg, c0, l16));
    }
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      bf16x8 b = cat(tr_read(hi, 4 * kg, 16 * j, l16), tr_read(hi, 16 + 4 * kg, 16 * j, l16));
      if (rem < 32) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if ((e < 4 ? 4 * kg + e : 12 + 4 * kg + e) >= rem) b[e] = static_cast<bf16>(0.f);
      }
      acc[0][j] = mfma16(a[0], b, acc[0][j]);  // D[column of A][column of H]
      acc[1][j] = mfma16(a[1], b, acc[1][j]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // ring consumed: the space takes the fp32 output tile
  float* tile = reinterpret_cast<float*>(smem);  // [128 columns of A][TS]
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[(32 * w + 16 * n + 4 * kg + r) * TS + 16 * j + l16] = acc[n][j][r];
  __syncthreads();
  float* ws = P.ws + ((int64_t)ks * P.nbt + pick(P.bo, pt)) * 128 * R;  // this product's plane of the split
  const int r4 = R / 4;
  if (!P.transpose) {  // ws[n][j]: thread -> 4 consecutive j of one n
    for (int e = tid; e < 128 * r4; e += 256) {
      const int n = e / r4, j4 = (e % r4) * 4;
      *reinterpret_cast<f32x4*>(ws + (int64_t)(nb * 128 + n) * R + j4) = *reinterpret_cast<const f32x4*>(&tile[n * TS + j4]);
    }
  } else {  // ws[j][n]: thread -> 4 consecutive n of one j
    for (int e = tid; e < 32 * R; e += 256) {
      const int j = e / 32, n4 = (e % 32) * 4;
      f32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = tile[(n4 + q) * TS + j];
      *reinterpret_cast<f32x4*>(ws + (int64_t)j * N + nb * 128 + n4) = v;
    }
  }
}

// out_t[row][col] (+)= alpha * sum_ks ws[ks][plane of t][row][col], rows x cols = N_t x R (or R x N_t
// transposed); grid y = product
__global__ __launch_bounds__(256) void tred_fin_kernel(const LoraTredParams P) {
  const int pt = blockIdx.y;
  const int N = pick(P.N, pt);
  const int64_t rows = P.transpose ? P.R : N, cols = P.transpose ? N : P.R;
  const int64_t n4 = rows * cols / 4, plane = (int64_t)P.nbt * 128 * P.R;
  const float* ws = P.ws + (int64_t)pick(P.bo, pt) * 128 * P.R;
  bf16* out = static_cast<bf16*>(pick(P.out, pt));
  const int64_t ldo = pick(P.ldo, pt);
  const bool acc = pick(P.accumulate, pt) != 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
    const int64_t row = (4 * e) / cols, col = (4 * e) % cols;
    f32x4 s = *reinterpret_cast<const f32x4*>(ws + 4 * e);
    for (int k = 1; k < P.ks; ++k) s += *reinterpret_cast<const f32x4*>(ws + k * plane + 4 * e);
    bf16x4* dst = reinterpret_cast<bf16x4*>(out + row * ldo + col);
    const bf16x4 old = acc ? *dst : bf16x4{};
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = static_cast<bf16>(P.alpha * s[q] + (acc ? static_cast<float>(old[q]) : 0.f));
    *dst = o;
  }
}

// ---------------------------------------------------------------------------------------------
// dx: dX[M][K] (+)= keep / (1 - p) (g[M][R] A[R][K]), from A^T [K][R]; R <= 32
// ---------------------------------------------------------------------------------------------
constexpr int DX_TS = 132;  // fp32 tile row: 128 + 4 so the f32x4 writes of 16 rows spread over banks

__global__ __launch_bounds__(256) void dx_kernel(const LoraDxParams P) {
  __shared__ __attribute__((aligned(16))) float tile[64 * DX_TS];
  const int tid = threadIdx.x, lane = tid & 63, kg = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkb = P.K / 128, R = P.R;
  const int64_t tb = blockIdx.x / nkb;
  const int kb = blockIdx.x % nkb;
  bf16* dx = static_cast<bf16*>(P.dx);
  const int64_t ldo = P.ld_out > 0 ? P.ld_out : (int64_t)P.K;
  const int64_t ldg = P.ldg > 0 ? P.ldg : (int64_t)R;
  bf16x8 old[4];  // the dX tile's 16-byte chunks, in flight during the product
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, row = c >> 4, col = (c & 15) * 8;
    const int64_t tok = tb * 64 + row;
    old[i] = bf16x8{};
    if (P.accumulate && tok < P.M) old[i] = *reinterpret_cast<const bf16x8*>(dx + tok * ldo + kb * 128 + col);
  }
  // wave w: tokens 16 w .. 16 w + 15 of the tile x the 8 column tiles; lane group kg holds ranks
  // 8 kg .. 8 kg + 7 of both operands, zero past R (the rank is the reduction index)
  const bool kin = 8 * kg < R;
  const int64_t tokc = min(tb * 64 + 16 * w + l16, P.M - 1);
  bf16x8 gf = bf16x8{};
  if (kin) gf = *reinterpret_cast<const bf16x8*>(static_cast<const bf16*>(P.g) + tokc * ldg + 8 * kg);
  const bf16* at = static_cast<const bf16*>(P.at) + ((int64_t)kb * 128 + l16) * R + 8 * kg;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    bf16x8 af = bf16x8{};
    if (kin) af = *reinterpret_cast<const bf16x8*>(at + (int64_t)16 * c * R);
    const f32x4 d = mfma16(af, gf, f32x4{0.f, 0.f, 0.f, 0.f});  // D[column][token]
    *reinterpret_cast<f32x4*>(&tile[(16 * w + l16) * DX_TS + 16 * c + 4 * kg]) = d;
  }
  __syncthreads();
  const bool drop = P.p > 0.f;
  const uint32_t thr = drop_thr(P.p);
  const float sc = drop ? 1.f / (1.f - P.p) : 1.f;
  const uint64_t key = hash_u64(P.seed);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, row = c >> 4, col = (c & 15) * 8;
    const int64_t t = tb * 64 + row;
    if (t >= P.M) continue;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(&tile[row * DX_TS + col]);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(&tile[row * DX_TS + col + 4]);
    const float d[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    bool kp[8];
    if (drop) keep8(key, P.offset + (uint64_t)t * (uint64_t)P.K + kb * 128 + col, thr, kp);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (drop && !kp[e]) ? 0.f : d[e] * sc;
      o[e] = static_cast<bf16>(static_cast<float>(old[i][e]) + v);
    }
    *reinterpret_cast<bf16x8*>(dx + t * ldo + kb * 128 + col) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// refresh: B_i [n_i][r] -> the adapter tail of W' and the B^T buffer (lora_refresh at r <= 32)
// ---------------------------------------------------------------------------------------------
// One workgroup = a 64-row slab of one B_i, staged in LDS so the B^T rows are written as 16-byte
// pieces of 128-byte runs.
__global__ __launch_bounds__(256) void refresh_kernel(const LoraRefreshParams P) {
  __shared__ bf16 tile[64][32 + 8];
  int j = 0, slab = blockIdx.x;
  while (j + 1 < P.ntarget && slab >= (P.n[j] + 63) / 64) { slab -= (P.n[j] + 63) / 64; ++j; }
  const bf16* B = static_cast<const bf16*>(P.b[j]);
  const int r0 = slab * 64, n = P.n[j], r = P.r, cpr = r / 8;
  bf16* W = static_cast<bf16*>(P.w);
  bf16* WT = static_cast<bf16*>(P.wt);
  for (int e = threadIdx.x; e < 64 * cpr; e += 256) {  // 64 rows x r / 8 chunks of 8 bf16
    const int rr = e / cpr, cc = (e % cpr) * 8;
    if (r0 + rr < n) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(B + (int64_t)(r0 + rr) * r + cc);
      *reinterpret_cast<bf16x8*>(W + (int64_t)(P.off[j] + r0 + rr) * P.ldw + P.col0 + j * r + cc) = v;
#pragma unroll
      for (int q = 0; q < 8; ++q) tile[rr][cc + q] = v[q];
    }
  }
  if (WT == nullptr) return;  // workgroup-uniform: no transposed copy wanted
  __syncthreads();
  for (int e = threadIdx.x; e < r * 8; e += 256) {  // B^T rows = the r columns of the slab (n % 8 == 0)
    const int cc = e >> 3, rr = (e & 7) * 8;
    if (r0 + rr < n) {
      bf16x8 v;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tile[rr + q][cc];
      *reinterpret_cast<bf16x8*>(WT + (int64_t)(P.trow0 + j * r + cc) * P.ldt + P.off[j] + r0 + rr) = v;
    }
  }
}

}  // namespace

bool lora_small_nt_supported(int64_t M, int K, int r) {
  return M > 0 && K > 0 && K % 128 == 0 && r % 8 == 0 && r >= 8 && r <= 48;
}

void lora_small_nt(const LoraSmallNtParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(((p.M + 31) / 32) * p.ks), (unsigned)p.nprod), block(256);
  const int rt = (p.r + 15) / 16, mode = p.p > 0.f ? (p.xd != nullptr ? 2 : 1) : 0;
#define GRT_LSNT(RT)                                                                                  \
  case RT:                                                                                            \
    if (mode == 0) hipLaunchKernelGGL((nt_kernel<RT, false, false>), grid, block, 0, s, p);           \
    else if (mode == 1) hipLaunchKernelGGL((nt_kernel<RT, true, false>), grid, block, 0, s, p);       \
    else hipLaunchKernelGGL((nt_kernel<RT, true, true>), grid, block, 0, s, p);                       \
    break;
  switch (rt) {
    GRT_LSNT(1) GRT_LSNT(2)
    default: GRT_LSNT(3)
  }
#undef GRT_LSNT
  if (p.ks > 1) {
    int64_t fb = (p.M * (p.r / 4) + 255) / 256;
    if (fb > 1024) fb = 1024;
    hipLaunchKernelGGL(nt_fin_kernel, dim3((unsigned)fb, (unsigned)p.nprod), block, 0, s, p);
  }
}

bool lora_small_tred_supported(int64_t M, int N, int R) {
  return M > 0 && N > 0 && N % 128 == 0 && R % 8 == 0 && R >= 8 && R <= 96;
}

// token splits: one workgroup per CU (lora_tred_splits' rule), at most 16, whole 32-token tiles
int lora_small_tred_splits(int64_t M, int N, int cus) {
  const int nblk = N / 128;
  int ks = (int)(((int64_t)cus + nblk - 1) / nblk);
  const int64_t tiles = (M + 31) / 32;
  if (ks > 16) ks = 16;
  if (ks > tiles) ks = (int)tiles;
  return ks < 1 ? 1 : ks;
}

void lora_small_tred(const LoraTredParams& p0, hipStream_t s) {
  LoraTredParams p = p0;
  const int64_t tiles = (p.M + 31) / 32;
  p.mchunk = 32 * ((tiles + p.ks - 1) / p.ks);
  const dim3 grid((unsigned)(p.nbt * p.ks)), block(256);
  switch ((p.R + 15) / 16) {
    case 1: hipLaunchKernelGGL(tred_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(tred_kernel<2>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(tred_kernel<3>, grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL(tred_kernel<4>, grid, block, 0, s, p); break;
    case 5: hipLaunchKernelGGL(tred_kernel<5>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(tred_kernel<6>, grid, block, 0, s, p); break;
  }
  int nmax = 0;
  for (int t = 0; t < p.nprod; ++t) nmax = p.N[t] > nmax ? p.N[t] : nmax;
  int64_t fb = ((int64_t)nmax * p.R / 4 + 255) / 256;
  if (fb > 1024) fb = 1024;
  hipLaunchKernelGGL(tred_fin_kernel, dim3((unsigned)fb, (unsigned)p.nprod), block, 0, s, p);
}

bool lora_small_dx_supported(int64_t M, int K, int R, uint64_t offset) {
  return M > 0 && K % 128 == 0 && R % 8 == 0 && R >= 8 && R <= 32 && offset % 4 == 0;
}

void lora_small_dx(const LoraDxParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(((p.M + 63) / 64) * (p.K / 128))), block(256);
  hipLaunchKernelGGL(dx_kernel, grid, block, 0, s, p);
}

void lora_small_refresh(const LoraRefreshParams& p, hipStream_t s) {
  int blocks = 0;
  for (int j = 0; j < p.ntarget; ++j) blocks += (p.n[j] + 63) / 64;
  hipLaunchKernelGGL(refresh_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
}

}  // namespace grt
