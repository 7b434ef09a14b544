// Flash attention for head_dim 64 in bf16 (forward + atomic-free backward) for gfx950 / CDNA4.
//
// Role: the 64-wide models (BasicLLM gpt2-small 768 / 12, Llama-3.2-1B 2048 / 32) train in bf16 on
// the same kind of kernel as the 128-wide ones (attention.hip, D = 128 only). Same contract, masks
// and dropout hash as attention.hip / attention_f32.hip / ops/_ref.attention, so the three families
// agree mask for mask. Through attn_fwd / attn_bwd, packing (cu_seqlens), the RoPE epilogue and the
// transposed side outputs stay with the D = 128 kernels; the 64-wide Llama path (RoPE inside the
// kernels, packing, dQKV epilogues on the fused QKV buffer) is rope_attention_d64.hip, built from
// the same tile helpers (grt_attn_d64.h).
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

#include "grt_attn_d64.h"
#include "grt_attn_dropout.h"
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

using namespace d64;  // tile geometry, MFMA / LDS helpers (grt_attn_d64.h)

// ------------------------------------------------------------------------------------------------
// Forward: 128 query rows per workgroup (32 per wave), 32-key tiles
// ------------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_fwd_d64_kernel(const AttnParams p) {
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * IMG];  // K[2] row-major, V[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (p.Sq + BM - 1) / BM;
  const int BH = p.B * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);  // heaviest causal blocks first
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  GRT_DEVICE_CHECK(b < p.B && hkv < p.Hkv && qblk >= 0);
  const int sk = p.seqlens_k ? min(p.Sk, p.seqlens_k[b]) : p.Sk;
  const int off = p.Sk - p.Sq;
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;

  const bf16* Q = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)hq * p.q_hs;
  const bf16* K = (const bf16*)p.k + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs;
  const bf16* V = (const bf16*)p.v + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs;

  bf16x8 qf[4];
  row_load(qf, Q + (int64_t)myq * p.q_ss, myq < p.Sq, h);

  int kend = sk;
  if (p.causal) kend = min(kend, q0 + BM + off);
  const int nt = kend > 0 ? (kend + TK - 1) / TK : 0;

  bf16x8 kreg, vreg;
  f32x16 o[2] = {f32x16{}, f32x16{}};
  float m = -INFINITY, l = 0.f;
  const float c = p.scale * kLog2e;

  if (nt > 0) {
    kreg = tile_load(K, p.k_ss, 0, sk);
    vreg = tile_load(V, p.v_ss, 0, sk);
    store_rm(kreg, smem);
    store_tr(vreg, smem + 2 * IMG);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vt = smem + (2 + cur) * IMG;
    if (t + 1 < nt) {
      kreg = tile_load(K, p.k_ss, kb + TK, sk);
      vreg = tile_load(V, p.v_ss, kb + TK, sk);
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
        const float e = fast_exp2(s[r] - msub);
        rs += e;  // normaliser over the undropped probabilities
        s[r] = DROP ? e * drop_factor(p, (uint32_t)bh, myq, kb + acc_row(r, h)) : e;
      }
      l = l * alpha + rs;
      m = mn;
      o[0] *= alpha;
      o[1] *= alpha;
      lds_t_x_acc(Vt, s, o, l32, h);
    }
    if (t + 1 < nt) {
      store_rm(kreg, smem + (cur ^ 1) * IMG);
      store_tr(vreg, smem + (2 + (cur ^ 1)) * IMG);
    }
    __syncthreads();
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (myq < p.Sq) {
    bf16* O = (bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)hq * p.o_hs + (int64_t)myq * p.o_ss;
    store_row(O, o, inv, h);
    if (h == 0 && p.lse)
      p.lse[((int64_t)b * p.Hq + hq) * p.Sq + myq] = lt > 0.f ? (m + __log2f(lt)) * kLn2 : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------
// delta[b,h,q] = sum_d dO*O: 8 lanes per row, one 16-byte chunk each
__global__ __launch_bounds__(256) void attn_bwd_pre_d64_kernel(const AttnBwdParams P) {
  const AttnParams& p = P.f;
  const int l8 = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int64_t nrows = (int64_t)p.B * p.Hq * p.Sq;
  float acc = 0.f;
  if (row < nrows) {
    const int q = (int)(row % p.Sq);
    const int64_t bh = row / p.Sq;
    const int hq = (int)(bh % p.Hq), b = (int)(bh / p.Hq);
    const bf16* O = (const bf16*)p.o + (int64_t)b * p.o_bs + (int64_t)hq * p.o_hs + (int64_t)q * p.o_ss;
    const bf16* dO = (const bf16*)P.dout + (int64_t)b * P.do_bs + (int64_t)hq * P.do_hs + (int64_t)q * P.do_ss;
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(O + l8 * 8);
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(dO + l8 * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += to_f(a[j]) * to_f(g[j]);
  }
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (row < nrows && l8 == 0) P.delta[row] = acc;
}

// dK / dV: 128 keys of one (batch, kv head) per workgroup, 32 per wave (key on the lane);
// sweeps the group's query heads x 32-row query tiles.
template <bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_bwd_dkdv_d64_kernel(const AttnBwdParams P) {
  const AttnParams& p = P.f;
  // Q[2] row-major, dO[2] row-major, Q[2] transposed, dO[2] transposed; lse[2], delta[2]
  __shared__ __attribute__((aligned(16))) bf16 smem[8 * IMG];
  __shared__ float stat[4 * TK];
  float* lsel = stat;
  float* dell = stat + 2 * TK;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BN = 128;
  const int nkb = (p.Sk + BN - 1) / BN;
  const int kblk = nkb - 1 - (int)(blockIdx.x / (p.B * p.Hkv));
  const int bhk = blockIdx.x % (p.B * p.Hkv);
  const int b = bhk / p.Hkv, hkv = bhk % p.Hkv;
  const int grp = p.Hq / p.Hkv;
  GRT_DEVICE_CHECK(kblk >= 0 && grp * p.Hkv == p.Hq);
  const int sk = p.seqlens_k ? min(p.Sk, p.seqlens_k[b]) : p.Sk;
  const int off = p.Sk - p.Sq;
  const int k0 = kblk * BN, kw0 = k0 + w * 32, mykey = kw0 + l32;
  const float c = p.scale * kLog2e;

  const bf16* K = (const bf16*)p.k + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs;
  const bf16* V = (const bf16*)p.v + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs;
  bf16x8 kf[4], vf[4];
  row_load(kf, K + (int64_t)mykey * p.k_ss, mykey < sk, h);
  row_load(vf, V + (int64_t)mykey * p.v_ss, mykey < sk, h);
  f32x16 dk[2] = {f32x16{}, f32x16{}}, dv[2] = {f32x16{}, f32x16{}};

  int qstart = p.causal ? max(0, k0 - off) : 0;
  qstart = (qstart / TK) * TK;
  const int nqt = qstart < p.Sq ? (p.Sq - qstart + TK - 1) / TK : 0;
  const int total = (k0 < sk) ? nqt * grp : 0;

  bf16x8 qreg, oreg;
  float lse_r = 0.f, del_r = 0.f;
  auto load_q = [&](int it) {
    const int hq = hkv * grp + it / nqt;
    const int qt = qstart + (it % nqt) * TK;
    const bf16* Q = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)hq * p.q_hs;
    const bf16* dO = (const bf16*)P.dout + (int64_t)b * P.do_bs + (int64_t)hq * P.do_hs;
    qreg = tile_load(Q, p.q_ss, qt, p.Sq);
    oreg = tile_load(dO, P.do_ss, qt, p.Sq);
    if (tid < TK) {
      const int q = qt + tid;
      const int64_t ri = ((int64_t)b * p.Hq + hq) * p.Sq + q;
      lse_r = q < p.Sq ? p.lse[ri] * kLog2e : INFINITY;
      del_r = q < p.Sq ? P.delta[ri] : 0.f;
    }
  };
  auto store_q = [&](int buf) {
    store_rm(qreg, smem + buf * IMG);
    store_rm(oreg, smem + (2 + buf) * IMG);
    store_tr(qreg, smem + (4 + buf) * IMG);
    store_tr(oreg, smem + (6 + buf) * IMG);
    if (tid < TK) { lsel[buf * TK + tid] = lse_r; dell[buf * TK + tid] = del_r; }
  };

  if (total > 0) { load_q(0); store_q(0); }
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
      const bool need_mask = (k0 + BN > sk) || (p.causal && kw0 + 31 > qt + off) || (qt + TK > p.Sq);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = acc_row(r, h), q = qt + qi;
        float pv = fast_exp2(s[r] * c - lsel[cur * TK + qi]);
        if (need_mask && (mykey >= sk || q >= p.Sq || (p.causal && mykey > q + off))) pv = 0.f;
        const float de = dell[cur * TK + qi];
        if (DROP) {
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

  if (mykey < p.Sk) {
    bf16* dK = (bf16*)P.dk + (int64_t)b * P.dk_bs + (int64_t)hkv * P.dk_hs + (int64_t)mykey * P.dk_ss;
    bf16* dV = (bf16*)P.dv + (int64_t)b * P.dv_bs + (int64_t)hkv * P.dv_hs + (int64_t)mykey * P.dv_ss;
    store_row(dK, dk, p.scale, h);
    store_row(dV, dv, 1.f, h);
  }
}

// dQ: the forward's structure; S^T and dP^T recomputed with the query on the lane,
// dQ^T += K^T dS^T with dS^T as the B operand.
template <bool DROP>
__global__ __launch_bounds__(NT, 2) void attn_bwd_dq_d64_kernel(const AttnBwdParams P) {
  const AttnParams& p = P.f;
  __shared__ __attribute__((aligned(16))) bf16 smem[6 * IMG];  // K[2], V[2] row-major, K[2] transposed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
  constexpr int BM = 128;
  const int nqb = (p.Sq + BM - 1) / BM;
  const int BH = p.B * p.Hq;
  const int qblk = nqb - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH;
  const int b = bh / p.Hq, hq = bh % p.Hq;
  const int hkv = hq / (p.Hq / p.Hkv);
  const int sk = p.seqlens_k ? min(p.Sk, p.seqlens_k[b]) : p.Sk;
  const int off = p.Sk - p.Sq;
  const int q0 = qblk * BM, qw0 = q0 + w * 32, myq = qw0 + l32;
  const bool qok = myq < p.Sq;

  const bf16* Q = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)hq * p.q_hs;
  const bf16* dO = (const bf16*)P.dout + (int64_t)b * P.do_bs + (int64_t)hq * P.do_hs;
  const bf16* K = (const bf16*)p.k + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs;
  const bf16* V = (const bf16*)p.v + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs;
  bf16x8 qf[4], of[4];
  row_load(qf, Q + (int64_t)myq * p.q_ss, qok, h);
  row_load(of, dO + (int64_t)myq * P.do_ss, qok, h);
  const int64_t ri = ((int64_t)b * p.Hq + hq) * p.Sq + (qok ? myq : 0);
  const float lse2 = qok ? p.lse[ri] * kLog2e : INFINITY;
  const float dlt = qok ? P.delta[ri] : 0.f;
  const float c = p.scale * kLog2e;

  int kend = sk;
  if (p.causal) kend = min(kend, q0 + BM + off);
  const int nt = kend > 0 ? (kend + TK - 1) / TK : 0;

  bf16x8 kreg, vreg;
  f32x16 dq[2] = {f32x16{}, f32x16{}};
  if (nt > 0) {
    kreg = tile_load(K, p.k_ss, 0, sk);
    vreg = tile_load(V, p.v_ss, 0, sk);
    store_rm(kreg, smem);
    store_rm(vreg, smem + 2 * IMG);
    store_tr(kreg, smem + 4 * IMG);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    const bf16* Kl = smem + cur * IMG;
    const bf16* Vl = smem + (2 + cur) * IMG;
    const bf16* Kt = smem + (4 + cur) * IMG;
    if (t + 1 < nt) {
      kreg = tile_load(K, p.k_ss, kb + TK, sk);
      vreg = tile_load(V, p.v_ss, kb + TK, sk);
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
        const float z = DROP ? drop_factor(p, (uint32_t)bh, myq, key) : 1.f;
        s[r] = pv * (dp[r] * z - dlt);
      }
      lds_t_x_acc(Kt, s, dq, l32, h);  // dQ^T += K^T dS^T
    }
    if (t + 1 < nt) {
      store_rm(kreg, smem + (cur ^ 1) * IMG);
      store_rm(vreg, smem + (2 + (cur ^ 1)) * IMG);
      store_tr(kreg, smem + (4 + (cur ^ 1)) * IMG);
    }
    __syncthreads();
  }
  if (qok) {
    bf16* dQ = (bf16*)P.dq + (int64_t)b * P.dq_bs + (int64_t)hq * P.dq_hs + (int64_t)myq * P.dq_ss;
    store_row(dQ, dq, p.scale, h);
  }
}

}  // namespace

bool attn_bf16_supported(int head_dim) { return head_dim == 64 || head_dim == 128; }

void attn_fwd_d64(const AttnParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(((p.Sq + 127) / 128) * p.B * p.Hq));
  if (p.drop_thresh) hipLaunchKernelGGL(attn_fwd_d64_kernel<true>, grid, dim3(NT), 0, s, p);
  else hipLaunchKernelGGL(attn_fwd_d64_kernel<false>, grid, dim3(NT), 0, s, p);
}

void attn_bwd_d64(const AttnBwdParams& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.f.B * p.f.Hq * p.f.Sq;
  hipLaunchKernelGGL(attn_bwd_pre_d64_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, s, p);
  const dim3 g1((unsigned)(((p.f.Sk + 127) / 128) * p.f.B * p.f.Hkv));
  const dim3 g2((unsigned)(((p.f.Sq + 127) / 128) * p.f.B * p.f.Hq));
  if (p.f.drop_thresh) {
    hipLaunchKernelGGL(attn_bwd_dkdv_d64_kernel<true>, g1, dim3(NT), 0, s, p);
    hipLaunchKernelGGL(attn_bwd_dq_d64_kernel<true>, g2, dim3(NT), 0, s, p);
  } else {
    hipLaunchKernelGGL(attn_bwd_dkdv_d64_kernel<false>, g1, dim3(NT), 0, s, p);
    hipLaunchKernelGGL(attn_bwd_dq_d64_kernel<false>, g2, dim3(NT), 0, s, p);
  }
}

}  // namespace grt
