// DoRA (weight-decomposed LoRA) kernels for gfx950 / CDNA4: the row norms of W + s B A without ever
// forming that matrix, the row scale y = c (.) u, and its backward with the magnitude gradient.
//
// Reference role: PEFT's ``LoraConfig(use_dora=True)`` on the adapted projections of the LoRA / QLoRA
// SFT job (peft/lora.py follows PEFT's names). Per target sub-projection i of an adapted module (rows
// off_i .. off_i + n_i of the fused base, A_i [r, in], B_i [n_i, r], magnitude m_i [n_i], s = scaling):
//     norm_j^2 = sum_k W_jk^2 + 2 s b_j . p_j + s^2 b_j^T G b_j,   p_j = (W A_i^T)_j,  G = A_i A_i^T
//     c_j = m_j / sqrt(max(norm_j^2, tiny))       (rows of no target: c = 1, norm reported as 1)
//     y = c (.) u                                  (u = the LoRA output, scaled in place)
//     du = c (.) dy,  dm_j = sum_t dy_tj y_tj / m_j   (u = y / c is not kept; m_j == 0: y == 0, dm_j = 0)
//
// norm (dora_norm_kernel): one launch per adapted module, W read once from where it lives: bf16 with
// any row stride (the head of the K-concatenated [W | B] buffer) or NF4 codes + fp32 absmax. The NF4
// decode is NOT gemm_nf4_skinny.hip's bf16(level) with the absmax on the accumulator: the training
// GEMM multiplies the dequantised bf16 W = bf16(level * absmax) (nf4.hip), and the norm has to be the
// norm of that matrix, so the absmax goes in before the rounding (fp32 levels in an LDS table
// replicated over the 32 banks, one ds_read_b32, one multiply and half a pack per weight).
// Work split: a workgroup owns 16 weight rows (out = 4096: 256 workgroups) of one slice; its 4 waves
// split the in axis in steps of 64 columns (one quant block). Lane (c = lane % 16, kg = lane / 16)
// holds the 16 columns 16 kg .. 16 kg + 15 of weight row c of the step: two 16-byte pieces (bf16) or
// one 8-byte load of codes, which are the B operands of two v_mfma_f32_16x16x32_bf16 whose A operands
// are the same columns of A_i row 16 jt + c (L2-resident; rows past r supply zeros: r = 8 is padded
// to the 16-wide rank tile in registers). D'[rank][weight row] puts weight row c in every lane, so the
// lane squares the same registers into that row's sum. The next step's loads are issued before the
// current one is consumed. The four partial [16 RT][16] tiles and row sums meet in LDS and are added
// in wave order; the epilogue, on all 256 threads, stages G_i and the 16 rows of B_i as fp32 in LDS
// and thread (row, slot) sums b_q (2 s p_q + s^2 (G b)_q) over q = slot, slot + 16, ..; 16 threads
// finish in slot order. No atomics: bitwise reproducible.
// The L2 traffic of A_i (r x in per workgroup, 4x the bf16 W bytes at r = 64) is the price of the
// 16-row split; more rows per workgroup would divide it and leave out = 4096 with under 256 workgroups.
// gram (dora_gram_kernel): G_i = A_i A_i^T in fp32, one workgroup per row, one wave per entry.
// scale (dora_scale_kernel): one read, one write, 16 bytes per thread.
// backward (dora_bwd_kernel + dora_dm_kernel): one pass over dy and y writes du and per-(token chunk)
// fp32 column partials; the second kernel adds the chunks in index order and divides by m.
#include "grt_common.h"
#include "grt_kernels.h"
#include "grt_nf4_table.h"

namespace grt {
namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <class T>
__device__ __forceinline__ T sel(const T (&v)[kDoraMaxTargets], int t) {
  return t == 0 ? v[0] : t == 1 ? v[1] : t == 2 ? v[2] : v[3];
}

// the target whose rows hold row n (-1: none); slices start and end on multiples of 16
__device__ __forceinline__ int target_of(const int (&off)[kDoraMaxTargets], const int (&n)[kDoraMaxTargets], int targets,
                                         int row) {
  int ti = -1;
#pragma unroll
  for (int i = 0; i < kDoraMaxTargets; ++i)
    if (i < targets && row >= off[i] && row < off[i] + n[i]) ti = i;
  return ti;
}

template <bool NF4, int RT>
struct Step {  // one 64-column step of a lane
  u32x2 q;
  float am;
  bf16x8 w[2];
  bf16x8 a[RT][2];
};

template <bool NF4, int RT>
__global__ __launch_bounds__(256) void dora_norm_kernel(const DoraNormParams P) {
  constexpr int LD = 16 * RT + 1;  // fp32 row of the epilogue's LDS tiles (odd: rows spread over banks)
  __shared__ __attribute__((aligned(2048))) float tab[16 * 32];
  __shared__ f32x4 red[4][RT][64];
  __shared__ float ssq[4][16];
  __shared__ float Gs[16 * RT * LD];
  __shared__ float Ps[16 * LD], Bs[16 * LD];
  __shared__ float part[16][17];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, kg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 16;
  const int ti = target_of(P.off, P.n, P.targets, n0);
  if (ti < 0) {  // workgroup-uniform: rows of an untargeted slice
    if (tid < 16) {
      P.c[n0 + tid] = 1.f;
      if (P.norm != nullptr) P.norm[n0 + tid] = 1.f;
    }
    return;
  }
  const int r = P.r, in = P.in, off = sel(P.off, ti);
  const float s = P.scaling;
  const bf16* __restrict__ A = static_cast<const bf16*>(sel(P.a, ti));
  const int64_t row = n0 + l16;
  const bf16* __restrict__ wr = NF4 ? nullptr : static_cast<const bf16*>(P.w) + row * P.ldw + kg * 16;
  const uint8_t* __restrict__ qr = NF4 ? P.q + ((row * in) >> 1) + kg * 8 : nullptr;
  const float* __restrict__ ar = NF4 ? P.absmax + row * (in >> 6) : nullptr;
  const int nsteps = in >> 6;
  auto load = [&](int t, Step<NF4, RT>& st) {
    if (NF4) {
      st.q = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(qr + t * 32));
      st.am = __builtin_nontemporal_load(ar + t);
    } else {
      st.w[0] = *reinterpret_cast<const bf16x8*>(wr + t * 64);
      st.w[1] = *reinterpret_cast<const bf16x8*>(wr + t * 64 + 8);
    }
#pragma unroll
    for (int jt = 0; jt < RT; ++jt) {
      st.a[jt][0] = bf16x8{}, st.a[jt][1] = bf16x8{};
      if (16 * jt + l16 < r) {
        const bf16* ap = A + (int64_t)(16 * jt + l16) * in + t * 64 + kg * 16;
        st.a[jt][0] = *reinterpret_cast<const bf16x8*>(ap);
        st.a[jt][1] = *reinterpret_cast<const bf16x8*>(ap + 8);
      }
    }
  };
  Step<NF4, RT> cur, nxt;
  int t = wave;
  if (t < nsteps) load(t, cur);
  if (NF4) {
    for (int i = tid; i < 16 * 32; i += 256) tab[i] = nf4_table::kLevels[i >> 5];
    __syncthreads();
  }
  f32x4 acc[RT];
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  while (t < nsteps) {
    const int tn = t + 4;
    if (tn < nsteps) load(tn, nxt);
    if (NF4) {  // element e of a word: byte e / 2, the high nibble first
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t wd = cur.q[h];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t code = (wd >> (8 * (e >> 1) + ((e & 1) ? 0 : 4))) & 15u;
          cur.w[h][e] = static_cast<bf16>(tab[(code << 5) + (lane & 31)] * cur.am);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = static_cast<float>(cur.w[h][e]);
        ss = fmaf(v, v, ss);
      }
#pragma unroll
      for (int jt = 0; jt < RT; ++jt)
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.a[jt][h], cur.w[h], acc[jt], 0, 0, 0);  // D'[rank][row]
    }
    cur = nxt;
    t = tn;
  }
  ss += __shfl_xor(ss, 16, kWave);
  ss += __shfl_xor(ss, 32, kWave);
  if (kg == 0) ssq[wave][l16] = ss;
#pragma unroll
  for (int jt = 0; jt < RT; ++jt) red[wave][jt][lane] = acc[jt];
  const float* __restrict__ G = P.g + (int64_t)ti * r * r;
  for (int e = tid; e < r * r; e += 256) Gs[(e / r) * LD + e % r] = G[e];
  const bf16* __restrict__ B = static_cast<const bf16*>(sel(P.b, ti)) + (int64_t)(n0 - off) * r;
  for (int e = tid; e < 16 * r; e += 256) Bs[(e / r) * LD + e % r] = static_cast<float>(B[e]);
  __syncthreads();
  for (int e = tid; e < RT * 256; e += 256) {  // P[row][rank], the waves' partials in wave order
    const int jt = e >> 8, ln = (e >> 2) & 63, q = e & 3;
    const float v = ((red[0][jt][ln][q] + red[1][jt][ln][q]) + red[2][jt][ln][q]) + red[3][jt][ln][q];
    Ps[(ln & 15) * LD + 16 * jt + 4 * (ln >> 4) + q] = v;
  }
  __syncthreads();
  {
    const int rw = tid & 15, slot = tid >> 4;
    float acc2 = 0.f;
    for (int q = slot; q < r; q += 16) {
      float gb = 0.f;
      for (int k = 0; k < r; ++k) gb = fmaf(Gs[q * LD + k], Bs[rw * LD + k], gb);
      acc2 += Bs[rw * LD + q] * (2.f * s * Ps[rw * LD + q] + s * s * gb);
    }
    part[rw][slot] = acc2;
  }
  __syncthreads();
  if (tid < 16) {
    float n2 = ((ssq[0][tid] + ssq[1][tid]) + ssq[2][tid]) + ssq[3][tid];
    float x = 0.f;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) x += part[tid][sl];
    n2 += x;
    const float nrm = sqrtf(fmaxf(n2, 1e-30f));
    const float m = static_cast<float>(static_cast<const bf16*>(sel(P.m, ti))[n0 - off + tid]);
    P.c[n0 + tid] = m / nrm;
    if (P.norm != nullptr) P.norm[n0 + tid] = nrm;
  }
}

// G_i[q][k] = A_i[q] . A_i[k] in fp32: grid (r, targets), wave w -> k = w, w + 4, ..
__global__ __launch_bounds__(256) void dora_gram_kernel(const DoraNormParams P) {
  const int q = blockIdx.x, ti = blockIdx.y, r = P.r, in = P.in;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bf16* __restrict__ A = static_cast<const bf16*>(sel(P.a, ti));
  const bf16* aq = A + (int64_t)q * in;
  for (int k = wave; k < r; k += 4) {
    const bf16* ak = A + (int64_t)k * in;
    float sum = 0.f;
    for (int c = lane * 8; c < in; c += 512) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(aq + c);
      const bf16x8 y = *reinterpret_cast<const bf16x8*>(ak + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum = fmaf(static_cast<float>(x[e]), static_cast<float>(y[e]), sum);
    }
    sum = wave_sum(sum);
    if (lane == 0) P.g[((int64_t)ti * r + q) * r + k] = sum;
  }
}

// y[t][j] = bf16(c[j] * y[t][j]), 8 columns per thread
__global__ __launch_bounds__(256) void dora_scale_kernel(bf16* __restrict__ y, int64_t ldy, const float* __restrict__ c,
                                                         int64_t M, int N) {
  const int n8 = N / 8;
  const int64_t total = M * n8;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / n8;
    const int j = (int)(e % n8) * 8;
    bf16x8* p = reinterpret_cast<bf16x8*>(y + m * ldy + j);
    const bf16x8 v = *p;
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(c + j), c1 = *reinterpret_cast<const f32x4*>(c + j + 4);
    bf16x8 o;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = static_cast<bf16>(static_cast<float>(v[q]) * (q < 4 ? c0[q] : c1[q - 4]));
    *p = o;
  }
}

// grid (column blocks of 128, token chunks): thread (cx = tid % 16, ry = tid / 16) owns 8 columns
// and every 16th token of the chunk; the 16 row-threads meet in LDS in ry order.
__global__ __launch_bounds__(256) void dora_bwd_kernel(const DoraBwdParams P) {
  __shared__ float sm[16][128 + 4];
  const int tid = threadIdx.x, cx = tid & 15, ry = tid >> 4;
  const int col = blockIdx.x * 128 + cx * 8;
  const bool valid = col < P.N;  // N % 8 == 0
  const int64_t mbeg = (int64_t)blockIdx.y * P.mchunk, mend = min(P.M, mbeg + P.mchunk);
  float sum[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) sum[q] = 0.f;
  if (valid) {
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(P.c + col), c1 = *reinterpret_cast<const f32x4*>(P.c + col + 4);
    const bf16* dy = static_cast<const bf16*>(P.dy);
    const bf16* y = static_cast<const bf16*>(P.y);
    bf16* du = static_cast<bf16*>(P.du);
    for (int64_t m = mbeg + ry; m < mend; m += 16) {
      const bf16x8 d = *reinterpret_cast<const bf16x8*>(dy + m * P.lddy + col);
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(y + m * P.ldy + col);
      bf16x8 o;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float df = static_cast<float>(d[q]);
        o[q] = static_cast<bf16>(df * (q < 4 ? c0[q] : c1[q - 4]));
        sum[q] = fmaf(df, static_cast<float>(v[q]), sum[q]);
      }
      *reinterpret_cast<bf16x8*>(du + m * P.lddu + col) = o;
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) sm[ry][cx * 8 + q] = sum[q];
  __syncthreads();
  if (tid < 128 && blockIdx.x * 128 + tid < P.N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sm[i][tid];
    P.ws[(int64_t)blockIdx.y * P.N + blockIdx.x * 128 + tid] = t;
  }
}

// dm[j] = (sum over the chunks, in order) / m_j for the columns of a target (m_j == 0: 0), else 0
__global__ __launch_bounds__(256) void dora_dm_kernel(const DoraBwdParams P) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= P.N) return;
  float t = 0.f;
  for (int k = 0; k < P.chunks; ++k) t += P.ws[(int64_t)k * P.N + j];
  const int ti = target_of(P.off, P.n, P.targets, j);
  float out = 0.f;
  if (ti >= 0) {
    const float m = static_cast<float>(static_cast<const bf16*>(sel(P.m, ti))[j - sel(P.off, ti)]);
    out = m != 0.f ? t / m : 0.f;
  }
  P.dm[j] = out;
}

template <bool NF4>
void launch_norm(const DoraNormParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(p.out / 16)), block(256);
  if (p.r <= 16) hipLaunchKernelGGL((dora_norm_kernel<NF4, 1>), grid, block, 0, s, p);
  else if (p.r == 32) hipLaunchKernelGGL((dora_norm_kernel<NF4, 2>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((dora_norm_kernel<NF4, 4>), grid, block, 0, s, p);
}

}  // namespace

bool dora_norm_supported(int out, int in, int r) {
  return out > 0 && out % 16 == 0 && in >= 64 && in % 64 == 0 && (r == 8 || r == 16 || r == 32 || r == 64);
}

void dora_norm(const DoraNormParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dora_gram_kernel, dim3((unsigned)p.r, (unsigned)p.targets), dim3(256), 0, s, p);
  if (p.q != nullptr) launch_norm<true>(p, s);
  else launch_norm<false>(p, s);
}

void dora_scale(void* y, int64_t ldy, const float* c, int64_t M, int N, hipStream_t s) {
  int64_t blocks = (M * (N / 8) + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(dora_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<bf16*>(y), ldy, c, M, N);
}

// token chunks: whole 16-token passes, about 1024 workgroups at most; a function of the shape alone
int dora_bwd_chunks(int64_t M, int N) {
  const int64_t passes = (M + 15) / 16, cb = (N + 127) / 128;
  int64_t ch = (1024 + cb - 1) / cb;
  if (ch > passes) ch = passes;
  return (int)(ch < 1 ? 1 : ch);
}

void dora_scale_bwd(const DoraBwdParams& p0, hipStream_t s) {
  DoraBwdParams p = p0;
  const int64_t passes = (p.M + 15) / 16;
  p.mchunk = 16 * ((passes + p.chunks - 1) / p.chunks);
  hipLaunchKernelGGL(dora_bwd_kernel, dim3((unsigned)((p.N + 127) / 128), (unsigned)p.chunks), dim3(256), 0, s, p);
  hipLaunchKernelGGL(dora_dm_kernel, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, s, p);
}

}  // namespace grt
