// Flash attention for head_dim 64 in bf16 (forward + atomic-free backward) for gfx950 / CDNA4, on
// separate q / k / v or, with RoPE inside and padding-free packing, on the fused QKV buffer.
//
// Role: the 64-wide models (BasicLLM gpt2-small 768 / 12, Llama-3.2-1B 2048 / 32) train in bf16 on
// the same kind of kernel as the 128-wide ones (attention.hip, D = 128 only). Same contract, masks
// and dropout hash as attention.hip / attention_f32.hip / ops/_ref.attention, so the three families
// agree mask for mask. Each of the four kernels (forward, delta pre-pass, dK/dV, dQ) is written once
// over a source policy that says where the operands live:
//   Plain (attn_fwd_d64 / attn_bwd_d64, AttnParams): strided q / k / v / o and their gradients,
//     seqlens_k, Sk >= Sq (causal offset Sk - Sq), dropout. Every block of the grid runs to its end;
//     one without keys has no tiles. Packing (cu_seqlens), the RoPE epilogue and the transposed side
//     outputs of attn_fwd / attn_bwd stay with the D = 128 kernels.
//   FusedRope (rope_attn_fwd_d64 / rope_attn_bwd_d64, RopeAttnD64Params): the 64-wide Llamas train
//     on one op per direction, like the 128-wide ones: qkv [T, (Hq + 2 Hkv) * 64] in, o [T, Hq * 64
//     (+ tail)] out, dqkv back, no rotated copy of q / k, no split / cat, one launch set for all
//     packed sequences. No dropout, causal offset 0. What the policy does differently:
//     RoPE on the load path. A lane's B operand is one half (d = 32 h .. + 31) of its own row and
//       the rotation partner d +- 32 is the other half of the same row, so whatever loads a Q / K
//       row or tile chunk also loads the partner chunk and the cos / sin row of its position,
//       rotates in fp32 and rounds once to bf16: that value is the MFMA operand and the LDS image.
//       V and dO are loaded as they are. Tile chunks are kept raw in registers across the tile's
//       math (the loads stay in flight) and rotated when they are stored to LDS.
//     Un-rotating epilogues. The dQ^T / dK^T accumulators hold d and d + 32 of the lane's row in
//       the same lane (acc[0][i], acc[1][i]), so the inverse rotation is lane-local; dQ / dK / dV
//       go straight into the Q / K / V columns of dqkv.
//     Packing. The grid is sized for the longest sequence; a workgroup whose block starts past the
//       end of its sequence returns before its first barrier (uniform per workgroup), so a block
//       that stays has at least one tile; every row bound (tile loads, masks, lse / delta, stores)
//       is the sequence's own length, so nothing is read from or written to a neighbouring
//       sequence's rows. Position = row index inside the sequence.
//
// Structure: that of attention_f32.hip with v_mfma_f32_32x32x16_bf16 (bf16 operands, fp32
// accumulate, fp32 softmax statistics; P and dS rounded to bf16 only as MFMA operands):
//   forward / dQ: per wave 32 query rows on the MFMA lane, K / V tiles of 32 keys double-buffered in
//     LDS; S^T = K Q^T (A = K rows from LDS, B = Q held in VGPRs), online softmax lane-local,
//     O^T += V^T P^T with the S^T accumulator as the B operand (cdna_hip_programming.md §3
//     "accumulator tile as the next MFMA's operand": element j of lane half h in k-step s is key
//     16 s + 8 (j >> 2) + 4 h + (j & 3)), the A side read from a transposed LDS image of the tile.
//   dK/dV: per wave 32 keys on the lane, K and V in VGPRs, Q / dO tiles of 32 rows in LDS;
//     S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS (no atomics).
// K-dim permutation of the QK^T / dO V^T products: MFMA step s reads d = 32 h + 8 s + j in lane
// half h, so one lane's A operand is one 16-byte LDS read of its row and its B operands are 32
// consecutive elements of its own row held in registers.
// LDS images (every element that is read is written by the tile store; pads are never read):
//   row-major  [32 rows][64 + 8]: 144-byte rows, the ds_read_b128 row reads of 16 consecutive rows
//     hit 16 distinct 4-bank quads;
//   transposed [64 d][32 + 4]: 72-byte rows, the two ds_read_b64 of a lane (keys 16 s + 4 h .. + 3
//     and + 8) are conflict-free across a 32-lane half (row pitch 18 dwords).
// The tile loader gives lanes 0..31 of a half-wave consecutive rows of one 16-byte column chunk, so
// the 2-byte stores of the transposed image are contiguous across the half-wave.
#include <stdlib.h>

#include "grt_attn_dropout.h"
#include "grt_common.h"
#include "grt_kernels.h"
#include "grt_mfma.h"

namespace grt {
namespace {

// ------------------------------------------------------------------------------------------------
// Tile geometry and MFMA / LDS building blocks: 4 waves, 32-row tiles, one 16-byte chunk per thread
// per tile, a row-major and a transposed LDS image
// ------------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------------
// RoPE on the load path, inverse RoPE in the epilogue, packed sequences (FusedRope)
// ------------------------------------------------------------------------------------------------
struct Seq {
  int64_t row0;  // first token row
  int len;
};
// clamped to the buffer and to S, so no index derived from it leaves qkv / o / lse
__device__ __forceinline__ Seq seq_of(const RopeAttnD64Params& p, int b) {
  if (!p.cu_seqlens) return {(int64_t)b * p.S, p.S};
  int64_t a = p.cu_seqlens[b], e = p.cu_seqlens[b + 1];
  a = a < 0 ? 0 : (a > p.T ? p.T : a);
  e = e > p.T ? p.T : e;
  const int64_t n = e - a;
  return {a, n < 0 ? 0 : (n > p.S ? p.S : (int)n)};
}

// this lane's half (d = 32 h .. + 31) of its own Q / K row, rotated at the row's position
// (cosr / sinr = that position's table rows): own * cos -+ partner * sin
__device__ __forceinline__ void row_load_rope(bf16x8 (&f)[4], const bf16* row, const float* cosr, const float* sinr,
                                              bool ok, int h) {
  const float sg = h ? 1.f : -1.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (ok) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(row + h * 32 + 8 * s);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(row + (h ^ 1) * 32 + 8 * s);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cosr + 8 * s + 4 * g);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(sinr + 8 * s + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          f[s][4 * g + j] = static_cast<bf16>(to_f(a[4 * g + j]) * c[j] + sg * to_f(b[4 * g + j]) * sn[j]);
      }
    } else {
      f[s] = zero8();
    }
  }
}

// this thread's chunk of a 32-row Q / K tile (row tid & 31, columns 8 ch .. + 7, ch = tid >> 5) with
// what its rotation needs: the partner chunk (ch ^ 4) and 8 cos / sin of the row's position
struct RopeChunk {
  bf16x8 own, par;
  f32x4 c0, c1, s0, s1;
};
__device__ __forceinline__ RopeChunk rope_tile_load(const bf16* src, int64_t ld, int r0, int rows_valid,
                                                    const float* cos, const float* sin) {
  const int row = threadIdx.x & 31, ch = threadIdx.x >> 5;
  const int gr = r0 + row;
  RopeChunk t;
  if (gr < rows_valid) {
    const bf16* x = src + (int64_t)gr * ld;
    t.own = *reinterpret_cast<const bf16x8*>(x + ch * 8);
    t.par = *reinterpret_cast<const bf16x8*>(x + (ch ^ 4) * 8);
    const int64_t ti = (int64_t)gr * 32 + (ch & 3) * 8;
    t.c0 = *reinterpret_cast<const f32x4*>(cos + ti);
    t.c1 = *reinterpret_cast<const f32x4*>(cos + ti + 4);
    t.s0 = *reinterpret_cast<const f32x4*>(sin + ti);
    t.s1 = *reinterpret_cast<const f32x4*>(sin + ti + 4);
  } else {
    t.own = t.par = zero8();
    t.c0 = t.c1 = t.s0 = t.s1 = f32x4{};
  }
  return t;
}
__device__ __forceinline__ bf16x8 rope_rotate(const RopeChunk& t) {
  const float sg = (threadIdx.x >> 7) ? 1.f : -1.f;  // chunk in the upper half of the row
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = static_cast<bf16>(to_f(t.own[j]) * t.c0[j] + sg * to_f(t.par[j]) * t.s0[j]);
    r[4 + j] = static_cast<bf16>(to_f(t.own[4 + j]) * t.c1[j] + sg * to_f(t.par[4 + j]) * t.s1[j]);
  }
  return r;
}

// store_row with the inverse rotation: acc[0][i] / acc[1][i] are d and d + 32 of the lane's row
__device__ __forceinline__ void store_row_unrope(bf16* dst, const f32x16 (&acc)[2], float mul, const float* cosr,
                                                 const float* sinr, int h) {
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
    const f32x4 c = *reinterpret_cast<const f32x4*>(cosr + 8 * gg + 4 * h);
    const f32x4 sn = *reinterpret_cast<const f32x4*>(sinr + 8 * gg + 4 * h);
    bf16x4 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a0 = acc[0][4 * gg + j] * mul, a1 = acc[1][4 * gg + j] * mul;
      v0[j] = static_cast<bf16>(a0 * c[j] + a1 * sn[j]);
      v1[j] = static_cast<bf16>(a1 * c[j] - a0 * sn[j]);
    }
    *reinterpret_cast<bf16x4*>(dst + 8 * gg + 4 * h) = v0;
    *reinterpret_cast<bf16x4*>(dst + 32 + 8 * gg + 4 * h) = v1;
  }
}

// ------------------------------------------------------------------------------------------------
// Source policies: where the operands of sequence b live and how a Q / K row gets in and out.
// Static functions over the kernel's params (Fwd; Bwd holds it as member f) and the sequence's own
// state (Seq): grid extents, row bounds, the causal offset, row addresses (x(head) = row 0 of that
// head, x_ld() its row stride, x_row(head, r) = row r), the Q / K loads (row, tile chunk and the
// value the chunk puts into LDS) and the dQ / dK row store.
// The params are taken by value on purpose. A field read through a reference to the kernel's params
// is loaded from a copy made at kernel entry, one read from the params or from a by-value argument
// where it is used; the second is what the kernels had before they shared one body, and the
// scheduler follows it (profiles/attn_d64_refactor.md). seq() alone keeps the reference that
// seq_of() always had.
// ------------------------------------------------------------------------------------------------
#define GRT_POLICY_FN static __device__ __forceinline__
struct Plain {
  typedef AttnParams Fwd;
  typedef AttnBwdParams Bwd;
  static constexpr bool kDropout = true;
  // every block runs to its end: a block without keys has no tiles, and lse is optional
  static constexpr bool kEarlyExit = false;
  struct Seq {
    int b, sk;  // batch row, keys that are attended to
  };
  static __host__ __device__ __forceinline__ int nseq(const Fwd p) { return p.B; }
  static __host__ __device__ __forceinline__ int qrows(const Fwd p) { return p.Sq; }  // grid extent, lse / delta pitch
  static __host__ __device__ __forceinline__ int krows(const Fwd p) { return p.Sk; }
  GRT_POLICY_FN Seq seq(const Fwd& p, int b) { return {b, p.seqlens_k ? min(p.Sk, p.seqlens_k[b]) : p.Sk}; }
  GRT_POLICY_FN int qlen(const Fwd p, Seq) { return p.Sq; }
  GRT_POLICY_FN int klen(const Fwd, Seq s) { return s.sk; }
  GRT_POLICY_FN int kstored(const Fwd p, Seq) { return p.Sk; }  // key rows whose dK / dV are written
  GRT_POLICY_FN int off(const Fwd p) { return p.Sk - p.Sq; }
  GRT_POLICY_FN bool wants_lse(const Fwd p) { return p.lse != nullptr; }
  GRT_POLICY_FN float* delta(const Bwd P) { return P.delta; }

  GRT_POLICY_FN const bf16* q(const Fwd p, Seq s, int hq) {
    return (const bf16*)p.q + (int64_t)s.b * p.q_bs + (int64_t)hq * p.q_hs;
  }
  GRT_POLICY_FN const bf16* k(const Fwd p, Seq s, int hkv) {
    return (const bf16*)p.k + (int64_t)s.b * p.k_bs + (int64_t)hkv * p.k_hs;
  }
  GRT_POLICY_FN const bf16* v(const Fwd p, Seq s, int hkv) {
    return (const bf16*)p.v + (int64_t)s.b * p.v_bs + (int64_t)hkv * p.v_hs;
  }
  GRT_POLICY_FN const bf16* dout(const Bwd P, Seq s, int hq) {
    return (const bf16*)P.dout + (int64_t)s.b * P.do_bs + (int64_t)hq * P.do_hs;
  }
  GRT_POLICY_FN int64_t q_ld(const Fwd p) { return p.q_ss; }
  GRT_POLICY_FN int64_t k_ld(const Fwd p) { return p.k_ss; }
  GRT_POLICY_FN int64_t v_ld(const Fwd p) { return p.v_ss; }
  GRT_POLICY_FN int64_t do_ld(const Bwd P) { return P.do_ss; }
  GRT_POLICY_FN const bf16* q_row(const Fwd p, Seq s, int hq, int r) { return q(p, s, hq) + (int64_t)r * p.q_ss; }
  GRT_POLICY_FN const bf16* k_row(const Fwd p, Seq s, int hkv, int r) { return k(p, s, hkv) + (int64_t)r * p.k_ss; }
  GRT_POLICY_FN const bf16* v_row(const Fwd p, Seq s, int hkv, int r) { return v(p, s, hkv) + (int64_t)r * p.v_ss; }
  GRT_POLICY_FN const bf16* dout_row(const Bwd P, Seq s, int hq, int r) {
    return dout(P, s, hq) + (int64_t)r * P.do_ss;
  }
  GRT_POLICY_FN bf16* o_row(const Fwd p, Seq s, int hq, int r) {
    return (bf16*)p.o + (int64_t)s.b * p.o_bs + (int64_t)hq * p.o_hs + (int64_t)r * p.o_ss;
  }
  GRT_POLICY_FN bf16* dq_row(const Bwd P, Seq s, int hq, int r) {
    return (bf16*)P.dq + (int64_t)s.b * P.dq_bs + (int64_t)hq * P.dq_hs + (int64_t)r * P.dq_ss;
  }
  GRT_POLICY_FN bf16* dk_row(const Bwd P, Seq s, int hkv, int r) {
    return (bf16*)P.dk + (int64_t)s.b * P.dk_bs + (int64_t)hkv * P.dk_hs + (int64_t)r * P.dk_ss;
  }
  GRT_POLICY_FN bf16* dv_row(const Bwd P, Seq s, int hkv, int r) {
    return (bf16*)P.dv + (int64_t)s.b * P.dv_bs + (int64_t)hkv * P.dv_hs + (int64_t)r * P.dv_ss;
  }

  typedef bf16x8 Chunk;
  struct Rot {};  // nothing to rotate with
  GRT_POLICY_FN Rot rot(const Fwd, int) { return {}; }
  GRT_POLICY_FN void load_row(bf16x8 (&f)[4], const bf16* row, Rot, bool ok, int h) { row_load(f, row, ok, h); }
  GRT_POLICY_FN Chunk load_tile(const Fwd, const bf16* src, int64_t ld, int r0, int rows_valid) {
    return tile_load(src, ld, r0, rows_valid);
  }
  GRT_POLICY_FN bf16x8 lds_value(Chunk t) { return t; }
  GRT_POLICY_FN void store_grad_row(bf16* dst, const f32x16 (&acc)[2], float mul, Rot, int h) {
    store_row(dst, acc, mul, h);
  }
};

struct FusedRope {
  typedef RopeAttnD64Params Fwd;
  struct Bwd {
    Fwd f;  // one struct serves both directions
  };
  static constexpr bool kDropout = false;
  // a block past the end of its sequence returns before its first barrier (uniform per workgroup):
  // a block that stays has at least one tile; lse is always written
  static constexpr bool kEarlyExit = true;
  typedef grt::Seq Seq;
  static __host__ __device__ __forceinline__ int nseq(const Fwd p) { return p.nseq; }
  static __host__ __device__ __forceinline__ int qrows(const Fwd p) { return p.S; }  // grid extent, lse / delta pitch
  static __host__ __device__ __forceinline__ int krows(const Fwd p) { return p.S; }
  GRT_POLICY_FN Seq seq(const Fwd& p, int b) { return seq_of(p, b); }
  GRT_POLICY_FN int qlen(const Fwd, Seq s) { return s.len; }
  GRT_POLICY_FN int klen(const Fwd, Seq s) { return s.len; }
  GRT_POLICY_FN int kstored(const Fwd, Seq s) { return s.len; }
  static constexpr __device__ __forceinline__ int off(const Fwd) { return 0; }
  GRT_POLICY_FN bool wants_lse(const Fwd) { return true; }
  GRT_POLICY_FN float* delta(const Bwd P) { return P.f.delta; }

  GRT_POLICY_FN const bf16* x(const Fwd p, Seq s) { return (const bf16*)p.qkv + s.row0 * p.ld; }
  GRT_POLICY_FN const bf16* q(const Fwd p, Seq s, int hq) { return x(p, s) + hq * D; }
  GRT_POLICY_FN const bf16* k(const Fwd p, Seq s, int hkv) { return x(p, s) + (p.Hq + hkv) * D; }
  GRT_POLICY_FN const bf16* v(const Fwd p, Seq s, int hkv) { return x(p, s) + (p.Hq + p.Hkv + hkv) * D; }
  GRT_POLICY_FN const bf16* dout(const Bwd P, Seq s, int hq) {
    return (const bf16*)P.f.dout + s.row0 * P.f.do_ld + hq * D;
  }
  GRT_POLICY_FN int64_t q_ld(const Fwd p) { return p.ld; }
  GRT_POLICY_FN int64_t k_ld(const Fwd p) { return p.ld; }
  GRT_POLICY_FN int64_t v_ld(const Fwd p) { return p.ld; }
  GRT_POLICY_FN int64_t do_ld(const Bwd P) { return P.f.do_ld; }
  GRT_POLICY_FN const bf16* q_row(const Fwd p, Seq s, int hq, int r) { return x(p, s) + (int64_t)r * p.ld + hq * D; }
  GRT_POLICY_FN const bf16* k_row(const Fwd p, Seq s, int hkv, int r) {
    return x(p, s) + (int64_t)r * p.ld + (p.Hq + hkv) * D;
  }
  GRT_POLICY_FN const bf16* v_row(const Fwd p, Seq s, int hkv, int r) {
    return x(p, s) + (int64_t)r * p.ld + (p.Hq + p.Hkv + hkv) * D;
  }
  GRT_POLICY_FN const bf16* dout_row(const Bwd P, Seq s, int hq, int r) {
    return (const bf16*)P.f.dout + (s.row0 + r) * P.f.do_ld + hq * D;
  }
  GRT_POLICY_FN bf16* o_row(const Fwd p, Seq s, int hq, int r) { return (bf16*)p.o + (s.row0 + r) * p.o_ld + hq * D; }
  GRT_POLICY_FN bf16* g_row(const Bwd P, Seq s, int r) { return (bf16*)P.f.dqkv + (s.row0 + r) * P.f.ld; }
  GRT_POLICY_FN bf16* dq_row(const Bwd P, Seq s, int hq, int r) { return g_row(P, s, r) + hq * D; }
  GRT_POLICY_FN bf16* dk_row(const Bwd P, Seq s, int hkv, int r) { return g_row(P, s, r) + (P.f.Hq + hkv) * D; }
  GRT_POLICY_FN bf16* dv_row(const Bwd P, Seq s, int hkv, int r) {
    return g_row(P, s, r) + (P.f.Hq + P.f.Hkv + hkv) * D;
  }

  typedef RopeChunk Chunk;
  struct Rot {
    const float* cosr;  // the table rows of one position
    const float* sinr;
  };
  GRT_POLICY_FN Rot rot(const Fwd p, int pos) { return {p.cos + (int64_t)pos * 32, p.sin + (int64_t)pos * 32}; }
  GRT_POLICY_FN void load_row(bf16x8 (&f)[4], const bf16* row, Rot r, bool ok, int h) {
    row_load_rope(f, row, r.cosr, r.sinr, ok, h);
  }
  GRT_POLICY_FN Chunk load_tile(const Fwd p, const bf16* src, int64_t ld, int r0, int rows_valid) {
    return rope_tile_load(src, ld, r0, rows_valid, p.cos, p.sin);
  }
  GRT_POLICY_FN bf16x8 lds_value(const Chunk& t) { return rope_rotate(t); }
  GRT_POLICY_FN void store_grad_row(bf16* dst, const f32x16 (&acc)[2], float mul, Rot r, int h) {
    store_row_unrope(dst, acc, mul, r.cosr, r.sinr, h);
  }
};
#undef GRT_POLICY_FN

// ------------------------------------------------------------------------------------------------
// Forward: 128 query rows per workgroup (32 per wave), 32-key tiles
// ------------------------------------------------------------------------------------------------
template <class Src, bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_fwd_d64_kernel(const typename Src::Fwd p) {
  static_assert(Src::kDropout || !DROP, "this source has no dropout");
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * IMG];  // K[2] row-major, V[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (Src::qrows(p) + BM - 1) / BM;
  const int BH = Src::nseq(p) * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);  // heaviest causal blocks first
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  GRT_DEVICE_CHECK(b < Src::nseq(p) && hkv < p.Hkv && qblk >= 0);
  const typename Src::Seq seq = Src::seq(p, b);
  const int sq = Src::qlen(p, seq), sk = Src::klen(p, seq);
  const int off = Src::off(p);
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;
  if constexpr (Src::kEarlyExit)
    if (q0 >= sq) return;

  const bf16* Q = Src::q(p, seq, hq);
  const bf16* K = Src::k(p, seq, hkv);
  const bf16* V = Src::v(p, seq, hkv);

  bf16x8 qf[4];
  Src::load_row(qf, Q + (int64_t)myq * Src::q_ld(p), Src::rot(p, myq), myq < sq, h);

  int kend = sk;
  if (p.causal) kend = min(kend, q0 + BM + off);
  const int nt = (Src::kEarlyExit || kend > 0) ? (kend + TK - 1) / TK : 0;

  typename Src::Chunk kraw;
  bf16x8 vreg;
  f32x16 o[2] = {f32x16{}, f32x16{}};
  float m = -INFINITY, l = 0.f;
  const float c = p.scale * kLog2e;

  if (Src::kEarlyExit || nt > 0) {
    kraw = Src::load_tile(p, K, Src::k_ld(p), 0, sk);
    vreg = tile_load(V, Src::v_ld(p), 0, sk);
    store_rm(Src::lds_value(kraw), smem);
    store_tr(vreg, smem + 2 * IMG);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vt = smem + (2 + cur) * IMG;
    if (t + 1 < nt) {
      kraw = Src::load_tile(p, K, Src::k_ld(p), kb + TK, sk);
      vreg = tile_load(V, Src::v_ld(p), kb + TK, sk);
    }
    if (!(p.causal && kb > qw0 + 31 + off)) {
      f32x16 s = rows_x_regs(Kl, qf, f32x16{}, l32, h);
      const bool need_mask = (kb + TK > sk) || (p.causal && kb + TK - 1 > qw0 + off);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = s[r] * c;
        if (need_mask) {
          const int key = kb + acc_row(r, h);
          if (key >= sk || (p.causal && key > myq + off)) v = -INFINITY;
        }
        s[r] = v;
        mx = fmaxf(mx, v);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      const float msub = (mn == -INFINITY) ? 0.f : mn;
      const float alpha = fast_exp2(m - msub);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float e = fast_exp2(s[r] - msub);
        rs += e;  // normaliser over the undropped probabilities
        if constexpr (DROP) e *= drop_factor(p, (uint32_t)bh, myq, kb + acc_row(r, h));
        s[r] = e;
      }
      l = l * alpha + rs;
      m = mn;
      o[0] *= alpha;
      o[1] *= alpha;
      lds_t_x_acc(Vt, s, o, l32, h);
    }
    if (t + 1 < nt) {
      store_rm(Src::lds_value(kraw), smem + (cur ^ 1) * IMG);
      store_tr(vreg, smem + (2 + (cur ^ 1)) * IMG);
    }
    __syncthreads();
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (myq < sq) {
    bf16* O = Src::o_row(p, seq, hq, myq);
    store_row(O, o, inv, h);
    if (h == 0 && Src::wants_lse(p))
      p.lse[((int64_t)b * p.Hq + hq) * Src::qrows(p) + myq] = lt > 0.f ? (m + __log2f(lt)) * kLn2 : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------
// delta[b,h,q] = sum_d dO*O for q inside sequence b: 8 lanes per row, one 16-byte chunk each
template <class Src>
__global__ __launch_bounds__(256) void attn_bwd_pre_d64_kernel(const typename Src::Bwd P) {
  const typename Src::Fwd& p = P.f;
  const int l8 = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int64_t nrows = (int64_t)Src::nseq(p) * p.Hq * Src::qrows(p);
  float acc = 0.f;
  bool ok = false;
  if (row < nrows) {
    const int q = (int)(row % Src::qrows(p));
    const int64_t bh = row / Src::qrows(p);
    const int hq = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
    const typename Src::Seq seq = Src::seq(p, b);
    ok = !Src::kEarlyExit || q < Src::qlen(p, seq);
    if (ok) {
      const bf16* O = Src::o_row(p, seq, hq, q);
      const bf16* dO = Src::dout_row(P, seq, hq, q);
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(O + l8 * 8);
      const bf16x8 g = *reinterpret_cast<const bf16x8*>(dO + l8 * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += to_f(a[j]) * to_f(g[j]);
    }
  }
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (ok && l8 == 0) Src::delta(P)[row] = acc;
}

// dK / dV: 128 keys of one (sequence, kv head) per workgroup, 32 per wave (key on the lane);
// sweeps the group's query heads x 32-row query tiles.
template <class Src, bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_bwd_dkdv_d64_kernel(const typename Src::Bwd P) {
  static_assert(Src::kDropout || !DROP, "this source has no dropout");
  const typename Src::Fwd& p = P.f;
  // Q[2] row-major, dO[2] row-major, Q[2] transposed, dO[2] transposed; lse[2], delta[2]
  __shared__ __attribute__((aligned(16))) bf16 smem[8 * IMG];
  __shared__ float stat[4 * TK];
  float* lsel = stat;
  float* dell = stat + 2 * TK;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BN = 128;
  const int nkb = (Src::krows(p) + BN - 1) / BN;
  const int kblk = nkb - 1 - (int)(blockIdx.x / (Src::nseq(p) * p.Hkv));
  const int bhk = blockIdx.x % (Src::nseq(p) * p.Hkv);
  const int b = bhk / p.Hkv, hkv = bhk % p.Hkv;
  const int grp = p.Hq / p.Hkv;
  GRT_DEVICE_CHECK(kblk >= 0 && grp * p.Hkv == p.Hq);
  const typename Src::Seq seq = Src::seq(p, b);
  const int sq = Src::qlen(p, seq), sk = Src::klen(p, seq);
  const int off = Src::off(p);
  const int k0 = kblk * BN, kw0 = k0 + w * 32, mykey = kw0 + l32;
  if constexpr (Src::kEarlyExit)
    if (k0 >= sk) return;
  const float c = p.scale * kLog2e;

  const typename Src::Rot rotk = Src::rot(p, mykey);
  bf16x8 kf[4], vf[4];
  Src::load_row(kf, Src::k_row(p, seq, hkv, mykey), rotk, mykey < sk, h);
  row_load(vf, Src::v_row(p, seq, hkv, mykey), mykey < sk, h);
  f32x16 dk[2] = {f32x16{}, f32x16{}}, dv[2] = {f32x16{}, f32x16{}};

  int qstart = p.causal ? (Src::kEarlyExit ? k0 : max(0, k0 - off)) : 0;
  qstart = (qstart / TK) * TK;
  const int nqt = (Src::kEarlyExit || qstart < sq) ? (sq - qstart + TK - 1) / TK : 0;
  const int total = (Src::kEarlyExit || k0 < sk) ? nqt * grp : 0;

  typename Src::Chunk qraw;
  bf16x8 oreg;
  float lse_r = 0.f, del_r = 0.f;
  auto load_q = [&](int it) {
    const int hq = hkv * grp + it / nqt;
    const int qt = qstart + (it % nqt) * TK;
    qraw = Src::load_tile(p, Src::q(p, seq, hq), Src::q_ld(p), qt, sq);
    oreg = tile_load(Src::dout(P, seq, hq), Src::do_ld(P), qt, sq);
    if (tid < TK) {
      const int q = qt + tid;
      const int64_t ri = ((int64_t)b * p.Hq + hq) * Src::qrows(p) + q;
      lse_r = q < sq ? p.lse[ri] * kLog2e : INFINITY;
      del_r = q < sq ? Src::delta(P)[ri] : 0.f;
    }
  };
  auto store_q = [&](int buf) {
    const bf16x8 qreg = Src::lds_value(qraw);
    store_rm(qreg, smem + buf * IMG);
    store_rm(oreg, smem + (2 + buf) * IMG);
    store_tr(qreg, smem + (4 + buf) * IMG);
    store_tr(oreg, smem + (6 + buf) * IMG);
    if (tid < TK) { lsel[buf * TK + tid] = lse_r; dell[buf * TK + tid] = del_r; }
  };

  if (Src::kEarlyExit || total > 0) { load_q(0); store_q(0); }
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    const int qt = qstart + (it % nqt) * TK;
    const uint32_t bhq = (uint32_t)(b * p.Hq + hkv * grp + it / nqt);
    if (it + 1 < total) load_q(it + 1);
    if (!(p.causal && kw0 > qt + TK - 1 + off)) {
      const bf16* Ql = smem + cur * IMG;
      const bf16* dOl = smem + (2 + cur) * IMG;
      const bf16* Qt = smem + (4 + cur) * IMG;
      const bf16* dOt = smem + (6 + cur) * IMG;
      f32x16 s = rows_x_regs(Ql, kf, f32x16{}, l32, h);
      f32x16 dp = rows_x_regs(dOl, vf, f32x16{}, l32, h);
      const bool need_mask = (k0 + BN > sk) || (p.causal && kw0 + 31 > qt + off) || (qt + TK > sq);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = acc_row(r, h), q = qt + qi;
        float pv = fast_exp2(s[r] * c - lsel[cur * TK + qi]);
        if (need_mask && (mykey >= sk || q >= sq || (p.causal && mykey > q + off))) pv = 0.f;
        const float de = dell[cur * TK + qi];
        if constexpr (DROP) {
          const float z = drop_factor(p, bhq, q, mykey);
          s[r] = pv * z;                  // dV sees the dropped probabilities
          dp[r] = pv * (dp[r] * z - de);
        } else {
          s[r] = pv;
          dp[r] = pv * (dp[r] - de);
        }
      }
      lds_t_x_acc(dOt, s, dv, l32, h);   // dV^T += dO^T P
      lds_t_x_acc(Qt, dp, dk, l32, h);   // dK^T += Q^T dS
    }
    if (it + 1 < total) store_q(cur ^ 1);
    __syncthreads();
  }

  if (mykey < Src::kstored(p, seq)) {
    bf16* dK = Src::dk_row(P, seq, hkv, mykey);
    bf16* dV = Src::dv_row(P, seq, hkv, mykey);
    Src::store_grad_row(dK, dk, p.scale, rotk, h);
    store_row(dV, dv, 1.f, h);
  }
}

// dQ: the forward's structure; S^T and dP^T recomputed with the query on the lane,
// dQ^T += K^T dS^T with dS^T as the B operand.
template <class Src, bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_bwd_dq_d64_kernel(const typename Src::Bwd P) {
  static_assert(Src::kDropout || !DROP, "this source has no dropout");
  const typename Src::Fwd& p = P.f;
  __shared__ __attribute__((aligned(16))) bf16 smem[6 * IMG];  // K[2], V[2] row-major, K[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (Src::qrows(p) + BM - 1) / BM;
  const int BH = Src::nseq(p) * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  const typename Src::Seq seq = Src::seq(p, b);
  const int sq = Src::qlen(p, seq), sk = Src::klen(p, seq);
  const int off = Src::off(p);
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;
  if constexpr (Src::kEarlyExit)
    if (q0 >= sq) return;
  const bool qok = myq < sq;

  const bf16* K = Src::k(p, seq, hkv);
  const bf16* V = Src::v(p, seq, hkv);
  const typename Src::Rot rotq = Src::rot(p, myq);
  bf16x8 qf[4], of[4];
  Src::load_row(qf, Src::q_row(p, seq, hq, myq), rotq, qok, h);
  row_load(of, Src::dout_row(P, seq, hq, myq), qok, h);
  const int64_t ri = ((int64_t)b * p.Hq + hq) * Src::qrows(p) + (qok ? myq : 0);
  const float lse2 = qok ? p.lse[ri] * kLog2e : INFINITY;
  const float dlt = qok ? Src::delta(P)[ri] : 0.f;
  const float c = p.scale * kLog2e;

  int kend = sk;
  if (p.causal) kend = min(kend, q0 + BM + off);
  const int nt = (Src::kEarlyExit || kend > 0) ? (kend + TK - 1) / TK : 0;

  typename Src::Chunk kraw;
  bf16x8 vreg;
  f32x16 dq[2] = {f32x16{}, f32x16{}};
  auto store_kv = [&](int buf) {
    const bf16x8 kreg = Src::lds_value(kraw);
    store_rm(kreg, smem + buf * IMG);
    store_rm(vreg, smem + (2 + buf) * IMG);
    store_tr(kreg, smem + (4 + buf) * IMG);
  };
  if (Src::kEarlyExit || nt > 0) {
    kraw = Src::load_tile(p, K, Src::k_ld(p), 0, sk);
    vreg = tile_load(V, Src::v_ld(p), 0, sk);
    store_kv(0);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vl = smem + (2 + cur) * IMG;
    const bf16* Kt = smem + (4 + cur) * IMG;
    if (t + 1 < nt) {
      kraw = Src::load_tile(p, K, Src::k_ld(p), kb + TK, sk);
      vreg = tile_load(V, Src::v_ld(p), kb + TK, sk);
    }
    if (!(p.causal && kb > qw0 + 31 + off)) {
      f32x16 s = rows_x_regs(Kl, qf, f32x16{}, l32, h);
      f32x16 dp = rows_x_regs(Vl, of, f32x16{}, l32, h);
      const bool need_mask = (kb + TK > sk) || (p.causal && kb + TK - 1 > qw0 + off);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + acc_row(r, h);
        float pv = fast_exp2(s[r] * c - lse2);
        if (need_mask && (key >= sk || (p.causal && key > myq + off))) pv = 0.f;
        float d = dp[r];
        if constexpr (DROP) d *= drop_factor(p, (uint32_t)bh, myq, key);
        s[r] = pv * (d - dlt);
      }
      lds_t_x_acc(Kt, s, dq, l32, h);  // dQ^T += K^T dS^T
    }
    if (t + 1 < nt) store_kv(cur ^ 1);
    __syncthreads();
  }
  if (qok) {
    bf16* dQ = Src::dq_row(P, seq, hq, myq);
    Src::store_grad_row(dQ, dq, p.scale, rotq, h);
  }
}

template <class Src, bool DROP>
void launch_fwd(const typename Src::Fwd& p, hipStream_t s) {
  const dim3 grid((unsigned)(((Src::qrows(p) + 127) / 128) * Src::nseq(p) * p.Hq));
  hipLaunchKernelGGL((attn_fwd_d64_kernel<Src, DROP>), grid, dim3(NT), 0, s, p);
}

template <class Src, bool DROP>
void launch_bwd(const typename Src::Bwd& P, hipStream_t s) {
  const typename Src::Fwd& p = P.f;
  const int64_t rows = (int64_t)Src::nseq(p) * p.Hq * Src::qrows(p);
  hipLaunchKernelGGL(attn_bwd_pre_d64_kernel<Src>, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, s, P);
  const dim3 g1((unsigned)(((Src::krows(p) + 127) / 128) * Src::nseq(p) * p.Hkv));
  const dim3 g2((unsigned)(((Src::qrows(p) + 127) / 128) * Src::nseq(p) * p.Hq));
  hipLaunchKernelGGL((attn_bwd_dkdv_d64_kernel<Src, DROP>), g1, dim3(NT), 0, s, P);
  hipLaunchKernelGGL((attn_bwd_dq_d64_kernel<Src, DROP>), g2, dim3(NT), 0, s, P);
}

}  // namespace

bool attn_bf16_supported(int head_dim) { return head_dim == 64 || head_dim == 128; }

void attn_fwd_d64(const AttnParams& p, hipStream_t s) {
  if (p.drop_thresh) launch_fwd<Plain, true>(p, s);
  else launch_fwd<Plain, false>(p, s);
}

void attn_bwd_d64(const AttnBwdParams& p, hipStream_t s) {
  if (p.f.drop_thresh) launch_bwd<Plain, true>(p, s);
  else launch_bwd<Plain, false>(p, s);
}

void rope_attn_fwd_d64(const RopeAttnD64Params& p, hipStream_t s) { launch_fwd<FusedRope, false>(p, s); }

void rope_attn_bwd_d64(const RopeAttnD64Params& p, hipStream_t s) { launch_bwd<FusedRope, false>(FusedRope::Bwd{p}, s); }

}  // namespace grt
