// Tile geometry and MFMA / LDS building blocks shared by the bf16 head_dim-64 attention kernels
// (attention_d64.hip, rope_attention_d64.hip): 4 waves, 32-row tiles, one 16-byte chunk per thread
// per tile, a row-major and a transposed LDS image. Layout notes: header of attention_d64.hip.
#pragma once
#include "grt_common.h"
#include "grt_mfma.h"

namespace grt {
namespace d64 {

constexpr int D = 64;
constexpr int NT = 256;        // 4 waves
constexpr int TK = 32;         // keys (fwd/dQ) or query rows (dK/dV) per LDS tile
constexpr int LDR = D + 8;     // row-major image pitch (bf16)
constexpr int LDT = TK + 4;    // transposed image pitch (bf16)
constexpr int IMG = TK * LDR;  // elements of either image
static_assert(IMG == D * LDT, "both images have the same size");
static_assert(TK * (D / 8) == NT, "one 16-byte chunk per thread per tile");
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = static_cast<bf16>(0.f);
  return z;
}

// this thread's chunk of a 32-row tile: row tid & 31, columns 8 (tid >> 5) .. + 7
__device__ __forceinline__ bf16x8 tile_load(const bf16* src, int64_t ld, int r0, int rows_valid) {
  const int row = threadIdx.x & 31, ch = threadIdx.x >> 5;
  const int gr = r0 + row;
  return gr < rows_valid ? *reinterpret_cast<const bf16x8*>(src + (int64_t)gr * ld + ch * 8) : zero8();
}
__device__ __forceinline__ void store_rm(bf16x8 reg, bf16* lds) {
  const int row = threadIdx.x & 31, ch = threadIdx.x >> 5;
  *reinterpret_cast<bf16x8*>(lds + row * LDR + ch * 8) = reg;
}
__device__ __forceinline__ void store_tr(bf16x8 reg, bf16* lds) {
  const int row = threadIdx.x & 31, ch = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 8; ++i) lds[(ch * 8 + i) * LDT + row] = reg[i];
}

// this lane's half (d = 32 h .. + 31) of its own row as the 4 B fragments of the row products
__device__ __forceinline__ void row_load(bf16x8 (&f)[4], const bf16* row, bool ok, int h) {
#pragma unroll
  for (int s = 0; s < 4; ++s) f[s] = ok ? *reinterpret_cast<const bf16x8*>(row + h * 32 + 8 * s) : zero8();
}

// acc += A(row-major tile in LDS, row = lane & 31) x B(this lane's own row), K = D
__device__ __forceinline__ f32x16 rows_x_regs(const bf16* lds, const bf16x8 (&b)[4], f32x16 acc, int l32, int h) {
  const bf16* row = lds + l32 * LDR + h * 32;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = mfma32(*reinterpret_cast<const bf16x8*>(row + 8 * s), b[s], acc);
  return acc;
}

// out[db] += (tile)^T[d][key] x P^T[key][lane]: P^T in the 32x32 accumulator `pt`, the tile's
// transposed image in LDS
__device__ __forceinline__ void lds_t_x_acc(const bf16* ldt, const f32x16& pt, f32x16 (&out)[2], int l32, int h) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 b = pack8(pt, 8 * s);
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const bf16* row = ldt + (db * 32 + l32) * LDT + 16 * s + 4 * h;
      const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(row);
      const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(row + 8);
      out[db] = mfma32(__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7), b, out[db]);
    }
  }
}

// store a 2 x f32x16 transposed accumulator (rows d, lane = this thread's row) as bf16 row `dst`
__device__ __forceinline__ void store_row(bf16* dst, const f32x16 (&acc)[2], float mul, int h) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = static_cast<bf16>(acc[db][4 * gg + j] * mul);
      *reinterpret_cast<bf16x4*>(dst + db * 32 + 8 * gg + 4 * h) = v;
    }
}

}  // namespace d64
}  // namespace grt
