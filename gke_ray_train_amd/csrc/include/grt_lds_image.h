// The XOR-swizzled bf16 LDS image shared by the attention, GEMM, LoRA and transposing kernels, with
// the accesses that go with it: transposed read, LDS-DMA fill, transposed tile store.
//
// Layout (cdna_hip_programming.md T10 (b)): [rows][128 x bf16], 256-byte rows (one LDS bank row) of
// sixteen 16-byte chunks; chunk ch of row `row` lives at chunk slot ch ^ swz(row), where
// swz(row) = ((row & 3) << 2) | ((row >> 2) & 3) is a bijection of row & 15. One image serves both
// access directions without bank conflicts:
//   * b128 row access (ds_read_b128 / ds_write_b128 / LDS-DMA of one chunk column over consecutive
//     rows): 16 consecutive rows have 16 distinct swz values, so the same chunk of those rows
//     lands in 16 distinct slots, all 64 banks once;
//   * ds_read_b64_tr_b16 column read: a 16-lane group reads 8-byte pieces of rows r0 .. r0 + 3 (r0 a
//     multiple of 4) from two adjacent chunks. The four rows differ in swz bits 2-3 and the two chunks
//     in bit 0, so the group covers 8 distinct slots, both halves of each: 32 banks. The other group
//     of the 32-lane half takes the other 32 when the caller gives it a row quad that differs in
//     (row >> 2) & 3 (swz bits 0-1).
#pragma once
#include "grt_common.h"

namespace grt {
namespace lds_image {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ int swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
// byte offset of 16-byte chunk `ch` of row `row`
__device__ __forceinline__ int chunk_off(int row, int ch) { return row * 256 + 16 * (ch ^ swz(row)); }

// transposed read: the 16-lane group reads rows r0 .. r0 + 3, columns c0 .. c0 + 15 (c0 a multiple
// of 16); lane i of the group receives column c0 + i of the 4 rows. EXEC must be all ones.
__device__ __forceinline__ bf16x4 tr_read(const char* base, int r0, int c0, int l16) {
  const int q = l16 >> 2, col = c0 + 4 * (l16 & 3);
  const char* a = base + chunk_off(r0 + q, col >> 3) + 8 * ((col >> 2) & 1);
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a);
}
__device__ __forceinline__ bf16x8 cat(bf16x4 a, bf16x4 b) {
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// LDS byte address of a generic pointer into __shared__ memory
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(p);
}

// 16-byte LDS-DMA per lane to (wave-uniform LDS byte address) + lane * 16. Inline asm, so hipcc's
// waitcnt pass does not track it (it would otherwise drain vmcnt in front of every LDS read of a
// pipelined loop): the calling kernel counts vmcnt itself. The destination base travels in M0:
//   * lds_dma16 writes M0 and names it as clobbered. That is sound only because M0 is
//     compiler-reserved and read in the same statement that writes it; the kernels whose hot loops
//     were scheduled and measured with this 3-instruction form keep it.
//   * lds_dma16_keep_m0 saves and restores M0 around the DMA, the recipe of cdna_hip_programming.md
//     §5.7; it assumes nothing about the compiler's use of M0. New code takes this one unless the two
//     extra SALU moves per DMA are measured to matter.
__device__ __forceinline__ void lds_dma16(const void* gptr, uint32_t lds_byte_addr) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               :: "v"(gptr), "s"(lds_byte_addr) : "memory", "m0");
}
__device__ __forceinline__ void lds_dma16_keep_m0(const void* gptr, uint32_t lds_byte_addr) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gptr), "s"(lds_byte_addr) : "memory");
}

// Epilogue of the kernels that also emit their 64 x 128 tile transposed (256 threads, after the
// barrier that follows the staging of the tile in `img`): image row r, column c goes to
// dst[(c0 + c) * ld + r0 + r]. Each 16-lane group takes two 16 x 16 blocks; 4 transposed reads give
// a lane 16 consecutive elements of one output row, stored as two 16-byte segments, so a wave
// stores 16 output rows x 128 bytes (full lines). I is the caller's index type, so that 32-bit
// index arithmetic stays 32-bit.
template <typename I>
__device__ __forceinline__ void store_transposed_64x128(const char* img, bf16* __restrict__ dst, I ld, I c0, I r0) {
  const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
#pragma unroll
  for (int pp = 0; pp < 2; ++pp) {
    const int pr = grp + 16 * pp;
    const int cb = 16 * (pr >> 2), rb = 16 * (pr & 3);  // 16 source columns, 16 source rows
    bf16x4 q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = tr_read(img, rb + 4 * k, cb, l16);
    bf16* d = dst + (int64_t)(c0 + cb + l16) * ld + r0 + rb;
    *reinterpret_cast<bf16x8*>(d) = cat(q[0], q[1]);
    *reinterpret_cast<bf16x8*>(d + 8) = cat(q[2], q[3]);
  }
}

}  // namespace lds_image
}  // namespace grt
