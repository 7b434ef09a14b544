// RoPE + flash attention for head_dim 64 in bf16 on the fused QKV buffer (forward + atomic-free
// backward), padding-free packed or not, for gfx950 / CDNA4.
//
// Role: the 64-wide Llamas (Llama-3.2-1B 2048 / 32) train on one op per direction, like the 128-wide
// ones: qkv [T, (Hq + 2 Hkv) * 64] in, o [T, Hq * 64 (+ tail)] out, dqkv back, no rotated copy of
// q / k, no split / cat, one launch set for all packed sequences.
//
// Structure: the kernels of attention_d64.hip (same tiles, LDS images and MFMA operand layouts,
// grt_attn_d64.h) with three changes:
//   RoPE on the load path. A lane's B operand is one half (d = 32 h .. + 31) of its own row and the
//     rotation partner d +- 32 is the other half of the same row, so whatever loads a Q / K row or
//     tile chunk also loads the partner chunk and the cos / sin row of its position, rotates in
//     fp32 and rounds once to bf16: that value is the MFMA operand and the LDS image. V and dO are
//     loaded as they are. Tile chunks are kept raw in registers across the tile's math (the loads
//     stay in flight) and rotated when they are stored to LDS.
//   Un-rotating epilogues. The dQ^T / dK^T accumulators hold d and d + 32 of the lane's row in the
//     same lane (acc[0][i], acc[1][i]), so the inverse rotation is lane-local; dQ / dK / dV go
//     straight into the Q / K / V columns of dqkv.
//   Packing. The grid is sized for the longest sequence; a workgroup whose block starts past the
//     end of its sequence returns before its first barrier (uniform per workgroup); every row bound
//     (tile loads, masks, lse / delta, stores) is the sequence's own length, so nothing is read from
//     or written to a neighbouring sequence's rows. Position = row index inside the sequence.
#include <stdlib.h>

#include "grt_attn_d64.h"
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

using namespace d64;
typedef RopeAttnD64Params Params;

struct Seq {
  int64_t row0;  // first token row
  int len;
};
// clamped to the buffer and to S, so no index derived from it leaves qkv / o / lse
__device__ __forceinline__ Seq seq_of(const Params& p, int b) {
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
// Forward: 128 query rows per workgroup (32 per wave), 32-key tiles
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 2) void rope_attn_fwd_d64_kernel(const Params p) {
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * IMG];  // K[2] row-major, V[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (p.S + BM - 1) / BM;
  const int BH = p.nseq * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);  // heaviest causal blocks first
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  GRT_DEVICE_CHECK(b < p.nseq && hkv < p.Hkv && qblk >= 0);
  const Seq sq = seq_of(p, b);
  const int len = sq.len;
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;
  if (q0 >= len) return;  // block past the end of this sequence (uniform, before any barrier)

  const bf16* X = (const bf16*)p.qkv + sq.row0 * p.ld;
  const bf16* Q = X + hq * D;
  const bf16* K = X + (p.Hq + hkv) * D;
  const bf16* V = X + (p.Hq + p.Hkv + hkv) * D;

  bf16x8 qf[4];
  row_load_rope(qf, Q + (int64_t)myq * p.ld, p.cos + (int64_t)myq * 32, p.sin + (int64_t)myq * 32, myq < len, h);

  const int kend = p.causal ? min(len, q0 + BM) : len;
  const int nt = (kend + TK - 1) / TK;  // >= 1: len > q0 >= 0

  RopeChunk kraw;
  bf16x8 vreg;
  f32x16 o[2] = {f32x16{}, f32x16{}};
  float m = -INFINITY, l = 0.f;
  const float c = p.scale * kLog2e;

  kraw = rope_tile_load(K, p.ld, 0, len, p.cos, p.sin);
  vreg = tile_load(V, p.ld, 0, len);
  store_rm(rope_rotate(kraw), smem);
  store_tr(vreg, smem + 2 * IMG);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vt = smem + (2 + cur) * IMG;
    if (t + 1 < nt) {
      kraw = rope_tile_load(K, p.ld, kb + TK, len, p.cos, p.sin);
      vreg = tile_load(V, p.ld, kb + TK, len);
    }
    if (!(p.causal && kb > qw0 + 31)) {
      f32x16 s = rows_x_regs(Kl, qf, f32x16{}, l32, h);
      const bool need_mask = (kb + TK > len) || (p.causal && kb + TK - 1 > qw0);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = s[r] * c;
        if (need_mask) {
          const int key = kb + acc_row(r, h);
          if (key >= len || (p.causal && key > myq)) v = -INFINITY;
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
        const float e = fast_exp2(s[r] - msub);
        rs += e;
        s[r] = e;
      }
      l = l * alpha + rs;
      m = mn;
      o[0] *= alpha;
      o[1] *= alpha;
      lds_t_x_acc(Vt, s, o, l32, h);
    }
    if (t + 1 < nt) {
      store_rm(rope_rotate(kraw), smem + (cur ^ 1) * IMG);
      store_tr(vreg, smem + (2 + (cur ^ 1)) * IMG);
    }
    __syncthreads();
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (myq < len) {
    bf16* O = (bf16*)p.o + (sq.row0 + myq) * p.o_ld + hq * D;
    store_row(O, o, inv, h);
    if (h == 0) p.lse[((int64_t)b * p.Hq + hq) * p.S + myq] = lt > 0.f ? (m + __log2f(lt)) * kLn2 : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------
// delta[b,h,q] = sum_d dO*O for q inside sequence b: 8 lanes per row, one 16-byte chunk each
__global__ __launch_bounds__(256) void rope_attn_bwd_pre_d64_kernel(const Params p) {
  const int l8 = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int64_t nrows = (int64_t)p.nseq * p.Hq * p.S;
  float acc = 0.f;
  bool ok = false;
  if (row < nrows) {
    const int q = (int)(row % p.S);
    const int64_t bh = row / p.S;
    const int hq = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
    const Seq sq = seq_of(p, b);
    ok = q < sq.len;
    if (ok) {
      const bf16* O = (const bf16*)p.o + (sq.row0 + q) * p.o_ld + hq * D;
      const bf16* dO = (const bf16*)p.dout + (sq.row0 + q) * p.do_ld + hq * D;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(O + l8 * 8);
      const bf16x8 g = *reinterpret_cast<const bf16x8*>(dO + l8 * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += to_f(a[j]) * to_f(g[j]);
    }
  }
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (ok && l8 == 0) p.delta[row] = acc;
}

// dK / dV: 128 keys of one (sequence, kv head) per workgroup, 32 per wave (key on the lane);
// sweeps the group's query heads x 32-row query tiles.
__global__ __launch_bounds__(NT, 2) void rope_attn_bwd_dkdv_d64_kernel(const Params p) {
  // Q[2] row-major, dO[2] row-major, Q[2] transposed, dO[2] transposed; lse[2], delta[2]
  __shared__ __attribute__((aligned(16))) bf16 smem[8 * IMG];
  __shared__ float stat[4 * TK];
  float* lsel = stat;
  float* dell = stat + 2 * TK;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BN = 128;
  const int nkb = (p.S + BN - 1) / BN;
  const int kblk = nkb - 1 - (int)(blockIdx.x / (p.nseq * p.Hkv));
  const int bhk = blockIdx.x % (p.nseq * p.Hkv);
  const int b = bhk / p.Hkv, hkv = bhk % p.Hkv;
  const int grp = p.Hq / p.Hkv;
  GRT_DEVICE_CHECK(kblk >= 0 && grp * p.Hkv == p.Hq);
  const Seq sq = seq_of(p, b);
  const int len = sq.len;
  const int k0 = kblk * BN, kw0 = k0 + w * 32, mykey = kw0 + l32;
  if (k0 >= len) return;  // block past the end of this sequence (uniform, before any barrier)
  const float c = p.scale * kLog2e;

  const bf16* X = (const bf16*)p.qkv + sq.row0 * p.ld;
  const bf16* dOb = (const bf16*)p.dout + sq.row0 * p.do_ld;
  const float* cosk = p.cos + (int64_t)mykey * 32;
  const float* sink = p.sin + (int64_t)mykey * 32;
  bf16x8 kf[4], vf[4];
  row_load_rope(kf, X + (int64_t)mykey * p.ld + (p.Hq + hkv) * D, cosk, sink, mykey < len, h);
  row_load(vf, X + (int64_t)mykey * p.ld + (p.Hq + p.Hkv + hkv) * D, mykey < len, h);
  f32x16 dk[2] = {f32x16{}, f32x16{}}, dv[2] = {f32x16{}, f32x16{}};

  const int qstart = p.causal ? (k0 / TK) * TK : 0;  // k0 < len
  const int nqt = (len - qstart + TK - 1) / TK;
  const int total = nqt * grp;

  RopeChunk qraw;
  bf16x8 oreg;
  float lse_r = 0.f, del_r = 0.f;
  auto load_q = [&](int it) {
    const int hq = hkv * grp + it / nqt;
    const int qt = qstart + (it % nqt) * TK;
    qraw = rope_tile_load(X + hq * D, p.ld, qt, len, p.cos, p.sin);
    oreg = tile_load(dOb + hq * D, p.do_ld, qt, len);
    if (tid < TK) {
      const int q = qt + tid;
      const int64_t ri = ((int64_t)b * p.Hq + hq) * p.S + q;
      lse_r = q < len ? p.lse[ri] * kLog2e : INFINITY;
      del_r = q < len ? p.delta[ri] : 0.f;
    }
  };
  auto store_q = [&](int buf) {
    const bf16x8 qreg = rope_rotate(qraw);
    store_rm(qreg, smem + buf * IMG);
    store_rm(oreg, smem + (2 + buf) * IMG);
    store_tr(qreg, smem + (4 + buf) * IMG);
    store_tr(oreg, smem + (6 + buf) * IMG);
    if (tid < TK) { lsel[buf * TK + tid] = lse_r; dell[buf * TK + tid] = del_r; }
  };

  load_q(0);
  store_q(0);
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    const int qt = qstart + (it % nqt) * TK;
    if (it + 1 < total) load_q(it + 1);
    if (!(p.causal && kw0 > qt + TK - 1)) {
      const bf16* Ql = smem + cur * IMG;
      const bf16* dOl = smem + (2 + cur) * IMG;
      const bf16* Qt = smem + (4 + cur) * IMG;
      const bf16* dOt = smem + (6 + cur) * IMG;
      f32x16 s = rows_x_regs(Ql, kf, f32x16{}, l32, h);
      f32x16 dp = rows_x_regs(dOl, vf, f32x16{}, l32, h);
      const bool need_mask = (k0 + BN > len) || (p.causal && kw0 + 31 > qt) || (qt + TK > len);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = acc_row(r, h), q = qt + qi;
        float pv = fast_exp2(s[r] * c - lsel[cur * TK + qi]);
        if (need_mask && (mykey >= len || q >= len || (p.causal && mykey > q))) pv = 0.f;
        const float de = dell[cur * TK + qi];
        s[r] = pv;
        dp[r] = pv * (dp[r] - de);
      }
      lds_t_x_acc(dOt, s, dv, l32, h);   // dV^T += dO^T P
      lds_t_x_acc(Qt, dp, dk, l32, h);   // dK^T += Q^T dS
    }
    if (it + 1 < total) store_q(cur ^ 1);
    __syncthreads();
  }

  if (mykey < len) {
    bf16* G = (bf16*)p.dqkv + (sq.row0 + mykey) * p.ld;
    store_row_unrope(G + (p.Hq + hkv) * D, dk, p.scale, cosk, sink, h);
    store_row(G + (p.Hq + p.Hkv + hkv) * D, dv, 1.f, h);
  }
}

// dQ: the forward's structure; S^T and dP^T recomputed with the query on the lane,
// dQ^T += K^T dS^T with dS^T as the B operand.
__global__ __launch_bounds__(NT, 2) void rope_attn_bwd_dq_d64_kernel(const Params p) {
  __shared__ __attribute__((aligned(16))) bf16 smem[6 * IMG];  // K[2], V[2] row-major, K[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (p.S + BM - 1) / BM;
  const int BH = p.nseq * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  const Seq sq = seq_of(p, b);
  const int len = sq.len;
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;
  if (q0 >= len) return;  // block past the end of this sequence (uniform, before any barrier)
  const bool qok = myq < len;

  const bf16* X = (const bf16*)p.qkv + sq.row0 * p.ld;
  const bf16* K = X + (p.Hq + hkv) * D;
  const bf16* V = X + (p.Hq + p.Hkv + hkv) * D;
  const float* cosq = p.cos + (int64_t)myq * 32;
  const float* sinq = p.sin + (int64_t)myq * 32;
  bf16x8 qf[4], of[4];
  row_load_rope(qf, X + (int64_t)myq * p.ld + hq * D, cosq, sinq, qok, h);
  row_load(of, (const bf16*)p.dout + (sq.row0 + myq) * p.do_ld + hq * D, qok, h);
  const int64_t ri = ((int64_t)b * p.Hq + hq) * p.S + (qok ? myq : 0);
  const float lse2 = qok ? p.lse[ri] * kLog2e : INFINITY;
  const float dlt = qok ? p.delta[ri] : 0.f;
  const float c = p.scale * kLog2e;

  const int kend = p.causal ? min(len, q0 + BM) : len;
  const int nt = (kend + TK - 1) / TK;  // >= 1

  RopeChunk kraw;
  bf16x8 vreg;
  f32x16 dq[2] = {f32x16{}, f32x16{}};
  auto store_kv = [&](int buf) {
    const bf16x8 kreg = rope_rotate(kraw);
    store_rm(kreg, smem + buf * IMG);
    store_rm(vreg, smem + (2 + buf) * IMG);
    store_tr(kreg, smem + (4 + buf) * IMG);
  };
  kraw = rope_tile_load(K, p.ld, 0, len, p.cos, p.sin);
  vreg = tile_load(V, p.ld, 0, len);
  store_kv(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vl = smem + (2 + cur) * IMG;
    const bf16* Kt = smem + (4 + cur) * IMG;
    if (t + 1 < nt) {
      kraw = rope_tile_load(K, p.ld, kb + TK, len, p.cos, p.sin);
      vreg = tile_load(V, p.ld, kb + TK, len);
    }
    if (!(p.causal && kb > qw0 + 31)) {
      f32x16 s = rows_x_regs(Kl, qf, f32x16{}, l32, h);
      f32x16 dp = rows_x_regs(Vl, of, f32x16{}, l32, h);
      const bool need_mask = (kb + TK > len) || (p.causal && kb + TK - 1 > qw0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + acc_row(r, h);
        float pv = fast_exp2(s[r] * c - lse2);
        if (need_mask && (key >= len || (p.causal && key > myq))) pv = 0.f;
        s[r] = pv * (dp[r] - dlt);
      }
      lds_t_x_acc(Kt, s, dq, l32, h);  // dQ^T += K^T dS^T
    }
    if (t + 1 < nt) store_kv(cur ^ 1);
    __syncthreads();
  }
  if (qok) {
    bf16* dQ = (bf16*)p.dqkv + (sq.row0 + myq) * p.ld + hq * D;
    store_row_unrope(dQ, dq, p.scale, cosq, sinq, h);
  }
}

}  // namespace

void rope_attn_fwd_d64(const RopeAttnD64Params& p, hipStream_t s) {
  const dim3 grid((unsigned)(((p.S + 127) / 128) * p.nseq * p.Hq));
  hipLaunchKernelGGL(rope_attn_fwd_d64_kernel, grid, dim3(NT), 0, s, p);
}

void rope_attn_bwd_d64(const RopeAttnD64Params& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.nseq * p.Hq * p.S;
  hipLaunchKernelGGL(rope_attn_bwd_pre_d64_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, s, p);
  const dim3 g1((unsigned)(((p.S + 127) / 128) * p.nseq * p.Hkv));
  const dim3 g2((unsigned)(((p.S + 127) / 128) * p.nseq * p.Hq));
  hipLaunchKernelGGL(rope_attn_bwd_dkdv_d64_kernel, g1, dim3(NT), 0, s, p);
  hipLaunchKernelGGL(rope_attn_bwd_dq_d64_kernel, g2, dim3(NT), 0, s, p);
}

}  // namespace grt
