// Flash-attention forward over the fp8 KV cache for gfx950 / CDNA4: the chunked prefill of
// generate(..., kv_cache_dtype="fp8"), S > 4 new tokens of a row on top of the n keys it holds.
//
// Contract (AttnPrefillFp8Params, grt_kernels.h): q bf16 [B, S, Hq, D] rotated, strided; kc / vc
// e4m3fn codes [B, n, Hkv, D] and k_scale / v_scale fp32 [B, n, Hkv], strided views of the cache
// (format: ops/_ref.py::kv_fp8_quantize, grt_fp8.h); the S query tokens are the last S of the n
// keys, token t attends keys [0, n - (S - 1 - t)): decode_attention.hip's token rule without its
// T <= 4 limit. o bf16 [B, S, Hq, D] contiguous. D = 128 or 64, Hq / Hkv in {1, 2, 4, 8}. One
// launch, no workspace: nothing O(n) is written to global memory.
//
// Work split: 256 threads, four waves, each wave one 32-row MFMA tile of query tokens of one q head.
// With gs = min(G, 4) (G = Hq / Hkv) wave w takes head w % gs of the workgroup's gs heads of one
// kv head and token tile w / gs of its 4 / gs tiles, so the K / V tile a workgroup converts serves
// the whole GQA group (G = 8: two workgroups of 4 heads per kv head): a code is loaded and
// converted once per workgroup, not once per q head. Grid: token blocks (heaviest first) x batch x
// kv head x G / gs.
//
// Load path: a 64-key tile is 64 x D codes of K and of V. Each thread loads its 8-code units as
// 8-byte words global -> registers (the cache rows are 8-byte aligned), v_cvt_pk_f32_fp8 widens
// them, they are packed to bf16 (exact: every finite e4m3fn value is a bf16 value) and written as
// one ds_write_b128 per unit into the swizzled image of grt_lds_image.h, 256-byte rows, one key per
// row (D = 64 uses the first eight chunk columns of a row; the swizzle spreads them over all
// sixteen slots). The image holds raw code values, never code x scale. The loads of tile i + 1 are
// issued before the MFMAs of tile i and stay in flight behind them; convert and ds_write follow the
// MFMAs into the other of two stages (K image + V image = 32 KiB per stage), one barrier per tile.
//
// Scales (the decode kernel's rule, profiles/kv_fp8.md): the tile's 64 K and 64 V scales go to LDS
// once, the K scale already times softmax_scale * log2(e). Score column j is multiplied by it in
// fp32 after the QK^T MFMA; the row sum l adds the unscaled p; the p that enters the PV MFMA is
// multiplied by v_scale[j] before it is rounded to bf16. No element of K or V is scaled on its own.
//
// MFMA mapping (that of attention.hip): S^T[key][q] = K Q^T with A = K rows from the image
// (ds_read_b128), B = the Q row of the lane held in registers for the whole key loop, so the row
// statistics of the base-2 online softmax (deferred rescale) are lane-local plus one permlane32 swap; O^T[d][q] +=
// V^T P^T with A = V^T by ds_read_b64_tr_b16 (tr_read) and B = the S^T accumulator packed in place
// (pack8).
//
// Causality and tails: key tiles wholly past the workgroup's last visible key are never loaded; a
// wave skips the math of tiles wholly past its own last key; tiles that touch the diagonal or the
// end of n are masked per element. Units and scales of keys >= n are not read (the registers hold
// code 0 and scale 0, so the image never keeps stale values), and no address leaves rows [0, n) of
// batch entry b. Query rows past S compute on the clamped row S - 1 and are not stored; a wave
// whose whole tile lies past S only keeps the barriers and its share of the loads.
#include "grt_common.h"
#include "grt_fp8.h"
#include "grt_kernels.h"
#include "grt_lds_image.h"
#include "grt_mfma.h"

namespace grt {
namespace {

using namespace lds_image;

constexpr int NT = 256;          // four waves
constexpr int TK = 64;           // keys per tile
constexpr int IMG = TK * 256;    // one image: 64 rows of 256 bytes
constexpr int STAGE = 2 * IMG;   // K image, V image
constexpr float kDeferLog2 = 8.f;

// max over lanes l and l ^ 32 by v_permlane32_swap (VALU, no LDS round trip)
__device__ __forceinline__ float halves_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// 8 codes -> the 16-byte bf16 chunk of the image
__device__ __forceinline__ bf16x8 codes_to_bf16(uint2 raw) {
  float f[8];
  fp8x8_to_f32(raw.x, raw.y, f);
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = static_cast<bf16>(f[i]);
  return v;
}

template <int D>
__global__ __launch_bounds__(NT, 2) void attn_prefill_fp8_kernel(const AttnPrefillFp8Params p) {
  constexpr int CPR = D / 8;            // 8-code units (16-byte image chunks) per key
  constexpr int RPI = NT / CPR;         // keys covered by one unit per thread
  constexpr int NU = TK / RPI;          // units per thread, tile and operand
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  __shared__ __attribute__((aligned(16))) float scl[2 * 2 * TK];  // [stage][K, V][key]

  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  const int g = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int G = p.Hq / p.Hkv;
  const int gs = G < 4 ? G : 4;         // heads per workgroup
  const int tiles = 4 / gs;             // 32-row token tiles per workgroup
  const int rows = 32 * tiles;
  const int nhg = G / gs;
  const int ntb = (p.S + rows - 1) / rows;
  const int per_tb = p.B * p.Hkv * nhg;
  const int tb = ntb - 1 - (int)(blockIdx.x / per_tb);  // heaviest token blocks first
  int rest = blockIdx.x % per_tb;
  const int hg = rest % nhg; rest /= nhg;
  const int hkv = rest % p.Hkv;
  const int b = rest / p.Hkv;
  GRT_DEVICE_CHECK(tb >= 0 && b < p.B && G * p.Hkv == p.Hq && gs * nhg == G);
  const int hq = hkv * G + hg * gs + w % gs;
  const int q0 = tb * rows, qw0 = q0 + (w / gs) * 32;
  const int off = p.n - p.S;            // token t sees keys <= t + off
  const int myq = min(qw0 + l32, p.S - 1);  // rows past S: the clamped row, not stored
  const int klim = myq + off;               // last key of this lane's row (< n)
  const int kmask = min(qw0, p.S - 1) + off + 1;  // tiles reaching past it need the mask
  // the wave's last visible key; -1: the whole tile lies past S, no math at all
  const int klast = qw0 < p.S ? min(qw0 + 31, p.S - 1) + off : -1;
  const int kend = min(q0 + rows - 1, p.S - 1) + off + 1;  // keys this workgroup reads, <= n
  const int nt = (kend + TK - 1) / TK;

  const uint8_t* Kg = (const uint8_t*)p.kc + (int64_t)b * p.k_bs + (int64_t)hkv * p.k_hs;
  const uint8_t* Vg = (const uint8_t*)p.vc + (int64_t)b * p.v_bs + (int64_t)hkv * p.v_hs;
  const float* Ksg = p.k_scale + (int64_t)b * p.ksc_bs + (int64_t)hkv * p.ksc_hs;
  const float* Vsg = p.v_scale + (int64_t)b * p.vsc_bs + (int64_t)hkv * p.vsc_hs;

  bf16x8 qf[D / 16];
  {
    const bf16* Q = (const bf16*)p.q + (int64_t)b * p.q_bs + (int64_t)myq * p.q_ss + (int64_t)hq * p.q_hs;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(Q + ks * 16 + 8 * h);
  }

  // this thread's units of a tile: key row ur + RPI * i, chunk uc. At D = 64 a 16-lane group holds
  // two keys; taking keys r and r + 2 (whose swizzles differ in bit 3) instead of r and r + 1
  // gives its ds_write_b128 sixteen distinct chunk slots.
  const int uc = tid % CPR;
  int ur = tid / CPR;
  if constexpr (D == 64) ur = (ur & ~3) | ((ur & 1) << 1) | ((ur >> 1) & 1);
  uint2 kraw[NU], vraw[NU];
  float sraw = 0.f;
  auto load_tile = [&](int t) {
    const int kb = t * TK;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int key = kb + ur + RPI * i;
      kraw[i] = vraw[i] = make_uint2(0u, 0u);
      if (key < p.n) {
        kraw[i] = *reinterpret_cast<const uint2*>(Kg + (int64_t)key * p.k_ss + uc * 8);
        vraw[i] = *reinterpret_cast<const uint2*>(Vg + (int64_t)key * p.v_ss + uc * 8);
      }
    }
    if (tid < 2 * TK) {  // waves 0 and 1: the K and the V scales of the tile
      const int key = kb + (tid & (TK - 1));
      sraw = 0.f;
      if (key < p.n) sraw = w == 0 ? Ksg[(int64_t)key * p.ksc_ss] : Vsg[(int64_t)key * p.vsc_ss];
    }
  };
  auto store_tile = [&](int stage) {
    char* ki = smem + stage * STAGE;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int o = chunk_off(ur + RPI * i, uc);
      *reinterpret_cast<bf16x8*>(ki + o) = codes_to_bf16(kraw[i]);
      *reinterpret_cast<bf16x8*>(ki + IMG + o) = codes_to_bf16(vraw[i]);
    }
    // the K scale times softmax_scale * log2(e), here and not at the load: the load stays in flight
    if (tid < 2 * TK) scl[stage * 2 * TK + tid] = w == 0 ? sraw * p.scale_log2 : sraw;
  };

  f32x16 o[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i) o[i] = f32x16{};
  float m = -INFINITY, l = 0.f;  // m in log2 units of the scaled scores

  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, kb = t * TK;
    if (t + 1 < nt) load_tile(t + 1);
    if (kb <= klast) {  // wave-uniform
      const char* ki = smem + cur * STAGE;
      const char* vi = ki + IMG;
      const float* ksl = scl + cur * 2 * TK;
      const float* vsl = ksl + TK;
      f32x16 s[2] = {f32x16{}, f32x16{}};
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ki + chunk_off(l32, 2 * ks + h));
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ki + chunk_off(32 + l32, 2 * ks + h));
        s[0] = mfma32(a0, qf[ks], s[0]);
        s[1] = mfma32(a1, qf[ks], s[1]);
      }
      // element r of s[blk] is key kb + 32 blk + acc_row(r, h): four runs of four consecutive keys
      const bool need_mask = kb + TK > kmask;
      float mx = -INFINITY;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int k0 = 32 * blk + 8 * g4 + 4 * h;
          const f32x4 ksc = *reinterpret_cast<const f32x4*>(ksl + k0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v = s[blk][4 * g4 + j] * ksc[j];
            if (need_mask && kb + k0 + j > klim) v = -INFINITY;
            s[blk][4 * g4 + j] = v;
            mx = fmaxf(mx, v);
          }
        }
      // Deferred rescale (attention.hip's rule): m moves only when some row of the wave sees a tile
      // max more than kDeferLog2 above it, so most tiles skip the O / l rescale; in between the
      // exponentials are bounded by 2^kDeferLog2 (exact in fp32 l / O, bf16 p keeps its relative
      // precision). Every row sees key 0 and tile 0 is never skipped: m is finite from tile 0 on.
      mx = halves_max(mx);
      if (__any(mx > m + kDeferLog2)) {
        const float mn = fmaxf(m, mx);
        const float alpha = fast_exp2(m - mn);  // first tile: m = -inf, alpha = 0 on l = O = 0
        l *= alpha;
#pragma unroll
        for (int db = 0; db < D / 32; ++db) o[db] *= alpha;
        m = mn;
      }
      float rs = 0.f;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 vsc = *reinterpret_cast<const f32x4*>(vsl + 32 * blk + 8 * g4 + 4 * h);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float e = fast_exp2(s[blk][4 * g4 + j] - m);
            rs += e;  // the normaliser adds the unscaled p
            s[blk][4 * g4 + j] = e * vsc[j];
          }
        }
      l += rs;
#pragma unroll
      for (int stp = 0; stp < 4; ++stp) {
        const bf16x8 pb = pack8(s[stp >> 1], 8 * (stp & 1));
        const int kk = 16 * stp + 4 * h;
#pragma unroll
        for (int db = 0; db < D / 32; ++db) {
          const int c0 = db * 32 + (g & 1) * 16;
          o[db] = mfma32(cat(tr_read(vi, kk, c0, l16), tr_read(vi, kk + 8, c0, l16)), pb, o[db]);
        }
      }
    }
    if (t + 1 < nt) store_tile(cur ^ 1);
    __syncthreads();
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  // O rows as 16-byte stores: lane l (h = 0) holds columns 8 gg .. + 3 of its row and lane l + 32
  // columns 8 gg + 4 .. + 7; one permlane32 swap per dword of the (gg, gg + 1) pair gives lanes
  // 0-31 columns 8 gg .. + 7 and lanes 32-63 the next eight. Every lane takes part in the swap.
  const bool mine = qw0 + l32 < p.S;
  bf16* O = (bf16*)p.o + (((int64_t)b * p.S + myq) * p.Hq + hq) * D;
#pragma unroll
  for (int db = 0; db < D / 32; ++db)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      union { bf16x4 v; uint32_t u[2]; } a, c;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a.v[j] = static_cast<bf16>(o[db][8 * gp + j] * inv);
        c.v[j] = static_cast<bf16>(o[db][8 * gp + 4 + j] * inv);
      }
      const auto r0 = __builtin_amdgcn_permlane32_swap(a.u[0], c.u[0], false, false);
      const auto r1 = __builtin_amdgcn_permlane32_swap(a.u[1], c.u[1], false, false);
      if (mine) *reinterpret_cast<uint4*>(O + db * 32 + 16 * gp + 8 * h) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
    }
}

template <int D>
void launch(const AttnPrefillFp8Params& p, hipStream_t s) {
  const int G = p.Hq / p.Hkv, gs = G < 4 ? G : 4;
  const int rows = 32 * (4 / gs);
  const int64_t grid = (int64_t)((p.S + rows - 1) / rows) * p.B * p.Hkv * (G / gs);
  hipLaunchKernelGGL(attn_prefill_fp8_kernel<D>, dim3((unsigned)grid), dim3(NT), 0, s, p);
}

}  // namespace

void attn_prefill_fp8(const AttnPrefillFp8Params& p, int head_dim, hipStream_t s) {
  if (p.B <= 0 || p.S <= 0) return;
  if (head_dim == 64) launch<64>(p, s);
  else launch<128>(p, s);
}

}  // namespace grt
