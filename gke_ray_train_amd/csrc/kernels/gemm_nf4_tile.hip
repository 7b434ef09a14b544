// Tile MFMA GEMM straight from NF4 codes, with an optional LoRA epilogue, for the 17-256 rows of a
// prefill chunk (the binding takes 1-256):
//   y[m][n] = bf16( sum_blocks absmax[n][blk] * sum_{k in blk} x[m][k] * bf16(level[q(n, k)])
//                   + s * sum_r' h[m][i r + r'] * B_i[n - off_i][r'] )               (row n in target i)
//
// Reference role: bitsandbytes' 4-bit GEMM under the prompt pass of HF ``generate`` (reference
// ray-jobs/fine_tune_llama_ray.py:138-146, 215-227). Without the dequant
// cache every prefill chunk used to rebuild a bf16 copy of every projection for the library GEMM
// (~4.5 B moved per weight where the codes are 0.5 B). The skinny kernel (gemm_nf4_skinny.hip) reads
// x again from L2 for every 16 weight rows; here x is staged once per 128 weight rows.
//
// Format and numerics: those of gemm_nf4_skinny.hip. Two codes per byte, element 2i in the high
// nibble, blocks of 64 share one fp32 absmax, K % 64 == 0; the weight operand is bf16(level) (RNE),
// sums inside a quant block are fp32, each block sum times the fp32 absmax goes into an fp32 running
// sum, one bf16 rounding at the end.
//
// Tile: a workgroup of 256 threads owns 128 weight rows x MT activation rows (MT in {32, 64, 128},
// the smallest that covers M; 129-256 rows are two row passes over grid.z) and one K range (grid.y).
// Waves: wave w owns weight rows 32 w .. 32 w + 31 of the tile and all MT rows. It decodes its B
// operand in registers from its own codes (grt_nf4_table.h), once per weight and workgroup pass, and
// feeds it to MT / 32 v_mfma_f32_32x32x16_bf16 per 16-k slice: the decode is amortised over them.
// Codes: lane (n = lane % 32, g = lane / 32) takes weight row n and, per quant block, the 16 bytes
// of k in [32 g, 32 g + 32): word j feeds MFMA j of the block. One K step is 4 quant blocks, a whole
// 128-byte line of the row; the loads are non-temporal and the next step's are issued before the
// current step is consumed.
// x: the step's [MT][256] slab is staged in LDS once per workgroup, by LDS-DMA, as two swizzled bf16
// images (grt_lds_image.h; image row = 128 k of one x row, rows [half][m]), double-buffered. Wave w
// stages the MT / 2 image rows from w * MT / 2, 4 rows per DMA. Rows >= M are zeroed once and never
// loaded; chunks past the end of the K range are never loaded and never read (their quant block is
// skipped, a wave-uniform branch). The A fragment of lane (m, g) for MFMA j is chunk
// 8 (blk & 1) + 4 g + j of image row (blk >> 1) MT + 32 t + m: the k the lane's code word holds.
// 16 consecutive m at one chunk hit 16 distinct slots, so the ds_read_b128 is conflict-free.
// One s_waitcnt vmcnt(0) and one barrier close a step: the DMA of the next slab and the next codes
// had the whole step to land.
// Absmax: D puts output column n in lane n % 32 of every accumulator register, so the block's absmax
// is one scalar per lane: per M tile, 4 MFMAs into a zeroed temporary, then acc = fma(absmax, tmp, acc).
// Split K: grid.y K ranges of whole quant blocks (the host picks them so that the grid fills the
// chip about once). One range: the workgroup writes bf16 y. More: each writes its fp32 partial tile
// into ws[split][M][N] and gemm_nf4_tile_reduce adds the splits in index order: no atomics, bitwise
// reproducible.
// LoRA epilogue (split 0): per M tile and target that the wave's 32 weight rows touch, r / 16
// (rounded up) more MFMAs into a second accumulator: A = h rows, columns of that target; B = the
// lane's own lora_B row, 8 r' per lane; lanes of another target, of bare rows or past r supply
// zeros. A column belongs to one target, every other target adds exact zeros to it, so the order of
// the target list does not change a bit. Then acc += s * acc_lora.
// Store: lane n % 32 holds one column: 2-byte (4-byte for a partial) stores, 32 consecutive n per row.
#include "grt_common.h"
#include "grt_kernels.h"
#include "grt_lds_image.h"
#include "grt_mfma.h"
#include "grt_nf4_table.h"

#include <algorithm>

namespace grt {
namespace {

using lds_image::lds_addr;
using lds_image::lds_dma16_keep_m0;
using lds_image::swz;
using nf4_table::decode8;

constexpr int kTileN = 128;    // weight rows of a workgroup
constexpr int kStepBlocks = 4; // quant blocks of a K step: one 128-byte line of codes per weight row
constexpr int kStepK = 64 * kStepBlocks;
constexpr int kMinSplitBlocks = 8;  // the host's choice gives no K range fewer quant blocks

struct TileArgs {
  const bf16* x;
  int64_t ldx;
  const uint8_t* q;
  const float* absmax;
  bf16* y;
  float* ws;   // [splits, M, N] partial tiles, null with one split
  int M, N, K;
  int per;     // k per split (the last split runs to K)
  // LoRA epilogue
  const bf16* h;  // [M, r * targets], row stride ldh
  int64_t ldh;
  int r, targets;
  float scaling;
  const bf16* b[kNf4GemvMaxTargets];  // lora_B [n_i, r] contiguous
  int off[kNf4GemvMaxTargets], n[kNf4GemvMaxTargets];
};

struct Codes {  // one K step of a lane: 16 bytes of codes and the absmax of kStepBlocks quant blocks
  u32x4 q[kStepBlocks];
  float am[kStepBlocks];
};

template <int MT, bool LORA>
__global__ __launch_bounds__(256) void gemm_nf4_tile_kernel(const TileArgs a) {
  constexpr int kTiles = MT / 32;      // M tiles of a wave
  constexpr int kBuf = 2 * MT * 256;   // bytes of one slab: two images of MT rows
  __shared__ __attribute__((aligned(2048))) uint32_t tab[16 * 32];
  extern __shared__ __attribute__((aligned(1024))) char slab[];  // [2][2][MT] image rows of 256 bytes
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = lane & 31, g = lane >> 5;
  const int M = a.M, N = a.N, K = a.K;
  const int m0 = blockIdx.z * MT;
  const int wn0 = blockIdx.x * kTileN + 32 * wave;  // first weight row of the wave
  const int k_lo = blockIdx.y * a.per;
  const int k_hi = blockIdx.y == gridDim.y - 1 ? K : k_lo + a.per;
  const int row = min(wn0 + n, N - 1);  // rows past N read row N - 1, never stored
  const uint8_t* __restrict__ qr = a.q + (((int64_t)row * K) >> 1) + 16 * g;
  const float* __restrict__ ar = a.absmax + (int64_t)row * (K >> 6);
  // blocks past the K range load nothing and are skipped
  auto load = [&](int k, Codes& c) {
#pragma unroll
    for (int u = 0; u < kStepBlocks; ++u) {
      const int kb = k + 64 * u;
      c.q[u] = u32x4{0u, 0u, 0u, 0u}, c.am[u] = 0.f;
      if (kb < k_hi) {
        c.q[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(qr + (kb >> 1)));
        c.am[u] = __builtin_nontemporal_load(ar + (kb >> 6));
      }
    }
  };
  // DMA i of wave w fills image rows w MT / 2 + 4 i .. + 3 of the slab: half w / 2 of the step, x rows
  // (w & 1) MT / 2 + 4 i + lane / 16. Slot lane % 16 of such a row holds chunk slot ^ swz(row), and
  // swz(row) = (lane / 16) << 2 | (i & 3) because MT / 2 is a multiple of 16.
  const int hb = wave >> 1;
  const int dm = m0 + (wave & 1) * (MT / 2) + (lane >> 4);
  const int dch = (lane & 15) ^ ((lane >> 4) << 2);
  const uint32_t slab0 = lds_addr(slab);
  auto stage = [&](int k, int buf) {
    const uint32_t d0 = slab0 + buf * kBuf + wave * (MT / 2) * 256;
#pragma unroll
    for (int i = 0; i < MT / 8; ++i) {
      const int m = dm + 4 * i;
      const int kk = k + 128 * hb + 8 * (dch ^ (i & 3));
      const uint32_t d = __builtin_amdgcn_readfirstlane(d0 + i * 1024);
      if (m < M && kk < k_hi) lds_dma16_keep_m0(a.x + (int64_t)m * a.ldx + kk, d);
    }
  };
  // the first step's loads are issued before the table is built and the idle rows are zeroed
  Codes cur, nxt;
  int k = k_lo, buf = 0;
  load(k, cur);
  stage(k, 0);
  nf4_table::fill<256>(tab);
  if (m0 + MT > M) {
    for (int c = threadIdx.x; c < 2 * 2 * MT * 16; c += 256)  // 16-byte chunks of both slabs
      if (m0 + ((c >> 4) & (MT - 1)) >= M) *reinterpret_cast<u32x4*>(slab + 16 * c) = u32x4{0u, 0u, 0u, 0u};
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const uint32_t col = nf4_table::column(tab, lane);
  const char* abase = slab + n * 256;
  const int asw = (4 * g) ^ swz(n);  // chunk c of the lane's row sits in slot c ^ swz(n); c = const | 4 g
  f32x16 acc[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  while (k < k_hi) {
    const int kn = k + kStepK;
    if (kn < k_hi) {
      load(kn, nxt);
      stage(kn, buf ^ 1);
    }
    const char* ab = abase + buf * kBuf;
#pragma unroll
    for (int u = 0; u < kStepBlocks; ++u) {
      if (k + 64 * u < k_hi) {
        bf16x8 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = decode8(cur.q[u][j], col);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
          f32x16 tmp;
#pragma unroll
          for (int r = 0; r < 16; ++r) tmp[r] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const char* p = ab + ((u >> 1) * MT + 32 * t) * 256 + 16 * ((8 * (u & 1) + j) ^ asw);
            tmp = mfma32(*reinterpret_cast<const bf16x8*>(p), b[j], tmp);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = fmaf(cur.am[u], tmp[r], acc[t][r]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next slab's DMA (the compiler does not count it)
    __syncthreads();
    cur = nxt;
    buf ^= 1;
    k = kn;
  }
  const int cn = wn0 + n;
  if constexpr (LORA) {
    if (blockIdx.y == 0) {
      const int r = a.r;
#pragma unroll
      for (int t = 0; t < kTiles; ++t) {
        const int m = m0 + 32 * t + n;  // as the A operand the lane is x row n of the M tile
        if (m0 + 32 * t >= M) break;
        f32x16 accl;
#pragma unroll
        for (int e = 0; e < 16; ++e) accl[e] = 0.f;
        // constant indices into the by-value arguments (scalar selects; gemv_nf4.hip)
#pragma unroll
        for (int i = 0; i < kNf4GemvMaxTargets; ++i) {
          if (i < a.targets && wn0 < a.off[i] + a.n[i] && wn0 + 32 > a.off[i]) {  // the wave touches target i
            const bool mine = cn >= a.off[i] && cn < a.off[i] + a.n[i];
            const bf16* bp = a.b[i] + (int64_t)(cn - a.off[i]) * r;
            const bf16* hp = a.h + (int64_t)m * a.ldh + i * r;
            for (int k0 = 0; k0 < r; k0 += 16) {
              const int kk = k0 + 8 * g;  // r % 8 == 0: a lane's 8 r' are all inside r or all past it
              bf16x8 av = bf16x8{}, bv = bf16x8{};
              if (m < M && kk < r) av = *reinterpret_cast<const bf16x8*>(hp + kk);
              if (mine && kk < r) bv = *reinterpret_cast<const bf16x8*>(bp + kk);
              accl = mfma32(av, bv, accl);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = fmaf(a.scaling, accl[e], acc[t][e]);
      }
    }
  }
  if (cn < N) {
    float* __restrict__ ws = a.ws ? a.ws + (int64_t)blockIdx.y * M * N : nullptr;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 32 * t + acc_row(r, g);
        if (m < M) {
          if (ws) ws[(int64_t)m * N + cn] = acc[t][r];
          else a.y[(int64_t)m * N + cn] = static_cast<bf16>(acc[t][r]);
        }
      }
    }
  }
}

// y = bf16(ws[0] + ws[1] + ... ), the splits in index order
__global__ __launch_bounds__(256) void gemm_nf4_tile_reduce(const float* __restrict__ ws, bf16* __restrict__ y,
                                                            int64_t mn, int splits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn) return;
  float v = ws[i];
  for (int s = 1; s < splits; ++s) v += ws[s * mn + i];
  y[i] = static_cast<bf16>(v);
}

template <int MT, bool LORA>
void launch_tile(const TileArgs& a, dim3 grid, hipStream_t s) {
  constexpr int kLds = 2 * 2 * MT * 256;  // above the 64 KiB a kernel gets without asking: once per device
  static bool asked[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !asked[dev])
    asked[dev] = hipFuncSetAttribute((const void*)gemm_nf4_tile_kernel<MT, LORA>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLds) == hipSuccess;
  hipLaunchKernelGGL((gemm_nf4_tile_kernel<MT, LORA>), grid, dim3(256), kLds, s, a);
}

int tile_rows(int M) { return M <= 32 ? 32 : M <= 64 ? 64 : 128; }

}  // namespace

Nf4TileSplit gemm_nf4_tile_split(int M, int N, int K, int k_split) {
  const int blocks = K / 64;
  if (k_split > 0) {  // the caller's: ceil(blocks / k_split) blocks each, refused when the last is empty
    const int per = (blocks + k_split - 1) / k_split;
    return (int64_t)(k_split - 1) * per < blocks ? Nf4TileSplit{k_split, per} : Nf4TileSplit{0, 0};
  }
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    return n;
  }();
  // tiles * splits * row passes fill the chip about once; no split under kMinSplitBlocks blocks
  const int mt = tile_rows(M);
  const int64_t wgs = (int64_t)((N + kTileN - 1) / kTileN) * ((M + mt - 1) / mt);
  const int want = (int)std::min<int64_t>(std::max<int64_t>(cus / wgs, 1), std::max(blocks / kMinSplitBlocks, 1));
  if (want == 1) return Nf4TileSplit{1, blocks};
  // whole K steps per split, so that every split starts on a 128-byte line of codes
  const int per = ((blocks + want - 1) / want + kStepBlocks - 1) / kStepBlocks * kStepBlocks;
  int splits = (blocks + per - 1) / per;
  if (splits > 1 && blocks - (splits - 1) * per < kMinSplitBlocks) --splits;  // the last split takes a short tail
  return Nf4TileSplit{splits, per};
}

void gemm_nf4_tile(const Nf4GemmTile& f, Nf4TileSplit split, float* ws, hipStream_t s) {
  TileArgs a{};
  a.x = static_cast<const bf16*>(f.x), a.ldx = f.ldx, a.q = f.q, a.absmax = f.absmax;
  a.y = static_cast<bf16*>(f.y), a.M = f.M, a.N = f.N, a.K = f.K;
  a.h = static_cast<const bf16*>(f.h), a.ldh = f.ldh, a.r = f.r, a.targets = f.targets, a.scaling = f.scaling;
  for (int i = 0; i < f.targets; ++i) a.b[i] = static_cast<const bf16*>(f.b[i]), a.off[i] = f.off[i], a.n[i] = f.n[i];
  const int k_split = split.splits;
  a.ws = k_split > 1 ? ws : nullptr;
  a.per = 64 * split.per;
  const int mt = tile_rows(f.M);
  const dim3 grid((unsigned)((f.N + kTileN - 1) / kTileN), (unsigned)k_split, (unsigned)((f.M + mt - 1) / mt));
  const bool lora = f.targets > 0;
  if (mt == 32) lora ? launch_tile<32, true>(a, grid, s) : launch_tile<32, false>(a, grid, s);
  else if (mt == 64) lora ? launch_tile<64, true>(a, grid, s) : launch_tile<64, false>(a, grid, s);
  else lora ? launch_tile<128, true>(a, grid, s) : launch_tile<128, false>(a, grid, s);
  if (k_split > 1) {
    const int64_t mn = (int64_t)f.M * f.N;
    hipLaunchKernelGGL(gemm_nf4_tile_reduce, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, s, ws, a.y, mn, k_split);
  }
}

}  // namespace grt
