// Register decode of NF4 codes into the bf16 operand of a matrix instruction, shared by the skinny
// and the tile GEMM from the codes (gemm_nf4_skinny.hip, gemm_nf4_tile.hip).
//
// The 16 levels, rounded to bf16 (RNE), sit in LDS replicated over the 32 banks: [16][32] 32-bit
// slots, the bf16 in the low half, written by every launch (`fill`). Lane l reads column l % 32, so
// the read is conflict-free for any codes. Per weight: shift, and-or (address), ds_read_b32 and half
// a shift-or (pack). The table must be 2 KiB-aligned in LDS.
#pragma once
#include "grt_common.h"

namespace grt {
namespace nf4_table {

static __constant__ float kLevels[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

// byte offset of the table row of the code at bits S .. S + 3 of w (a row is 32 slots = 128 bytes)
template <int S>
__device__ __forceinline__ uint32_t row_off(uint32_t w) {
  return (S >= 7 ? w >> (S >= 7 ? S - 7 : 0) : w << (S < 7 ? 7 - S : 0)) & 0x780u;
}

// The table is 2 KiB-aligned in LDS, so a slot's address is (row offset) | col with col = the LDS
// address of the lane's column in row 0: one v_and_or_b32 (as pointer + offset the compiler emits
// an and and an add).
typedef __attribute__((address_space(3))) const uint32_t* LdsSlot;

// written by all NT threads of the workgroup; the caller's barrier follows
template <int NT>
__device__ __forceinline__ void fill(uint32_t* tab) {
  for (int i = threadIdx.x; i < 16 * 32; i += NT)
    tab[i] = __builtin_bit_cast(unsigned short, static_cast<bf16>(kLevels[i >> 5]));
}
__device__ __forceinline__ uint32_t column(const uint32_t* tab, int lane) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsSlot)(tab + (lane & 31))));
}

// 8 codes (one 32-bit word: byte j holds element 2j in its high nibble, 2j + 1 in its low) -> 8 bf16
template <int J>
__device__ __forceinline__ uint32_t decode2(uint32_t w, uint32_t col) {
  const uint32_t e = *reinterpret_cast<LdsSlot>(row_off<8 * J + 4>(w) | col);
  const uint32_t o = *reinterpret_cast<LdsSlot>(row_off<8 * J>(w) | col);
  return e | (o << 16);
}
__device__ __forceinline__ bf16x8 decode8(uint32_t w, uint32_t col) {
  const u32x4 d = {decode2<0>(w, col), decode2<1>(w, col), decode2<2>(w, col), decode2<3>(w, col)};
  return __builtin_bit_cast(bf16x8, d);
}

}  // namespace nf4_table
}  // namespace grt
