// Token sampler for the decode step: one launch picks one token per row of logits [B, V] (greedy,
// temperature, top-k, top-p) and does the generate() loop's bookkeeping (pad after EOS, finished
// flags, the next replay's embedding input, the output column), so a captured decode step needs
// no torch op between two replays. ops/_ref.py::sample_tokens is the host implementation.
//
// Semantics (fp32 unless noted):
//   z_i = logit_i * (1 / T), one fp32 multiply by the fp32 reciprocal the host computed; NaN counts
//   as -inf. Greedy is the argmax of the raw logits, lowest index on ties.
//   top-k keeps i iff #{j : z_j > z_i} < k; top-p keeps a top-k survivor i iff M_>(i) < top_p * Z
//   with e_j = exp(z_j - z_max), Z the survivors' sum and M_>(i) the sum over survivors with
//   z_j > z_i. Both kept sets are {z >= threshold}, so ties stay or go together and the maximum
//   always stays. -inf is never kept.
//   Draw: argmax over the kept set of z_i + g_i (Gumbel-max), lowest index on ties.
//
// Noise recipe (mirrored by _ref.sample_noise):
//   key = hash_u64(hash_u64(seed) + counter)                (64-bit wrapping add)
//   h_i = hash_u64(key ^ ((row << 32) | i))                 (i < 2^31)
//   n_i = h_i >> 41 (the top 23 bits), u_i = (n_i + 0.5) * 2^-23 (exact in fp32, inside (0, 1))
//   g_i = -log(-log(u_i))
// Noise is generated in the final pass only, for kept elements only.
//
// Candidate mode (speculative decoding): the rows of logits [T, V] are consecutive tokens of one
// sequence; row t uses counter + t and noise row 0, i.e. it draws what a one-row call draws at
// that token number, and only tokens[t] is written.
//
// Threshold search: no sort. z maps to a 32-bit key that orders like z; a radix select walks the
// key in digits of 11 / 11 / 10 bits, one pass over the row (from L2) per digit, each pass filling
// one LDS histogram with integer atomics: element counts for top-k, and for top-p the masses e_j
// in 64-bit fixed point (e_j <= 1 scaled by 2^40, or less for V > 2^22 so V addends cannot
// overflow). Integer sums do not depend on the order of arrival, so the kept set is bitwise
// reproducible. A block-wide scan from the top bin finds the bin where the running count / mass
// crosses the target, which becomes the next prefix.
//
// One workgroup of 1024 threads per row; nothing a workgroup writes is read by another one.
// Passes over the row: greedy 1, temperature only 1, top-k 3 + 1, top-p 1 + 3 + 1, both 3 + 3 + 1
// (fewer when a bin boundary hits the target exactly).
#include <hip/hip_runtime.h>

#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

constexpr int kNT = 1024;
constexpr int kWaves = kNT / kWave;
constexpr int kBins = 2048;  // 11-bit digit; 2 bins per thread in the scan
static_assert(kBins == 2 * kNT, "select_bin: two bins per thread");

typedef unsigned long long u64;

struct Best {
  float s;
  int i;
};
__device__ __forceinline__ void best_take(Best& a, float s, int i) {
  if (s > a.s || (s == a.s && i < a.i)) a.s = s, a.i = i;  // NaN never enters
}

struct Shared {
  u64 hist[kBins];
  u64 wtot[kWaves];
  float red_s[kWaves];
  int red_i[kWaves];
  u64 sel_above;
  int sel_bin;    // -1: no bin crossed the target
  int sel_exact;  // the bin's inclusive sum equals the target: the whole bin is kept
};

// f(i, x) for every element of the row. 16-byte loads over the aligned body, scalar head / tail,
// so a row may start at any element (padded strides, V not a multiple of the vector).
template <typename T, typename F>
__device__ __forceinline__ void for_row(const T* __restrict__ row, int V, F&& f) {
  constexpr int N = Vec16<T>::N;
  const int tid = threadIdx.x;
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / sizeof(T));
  if (head > V) head = V;
  if (tid < head) f(tid, to_f(row[tid]));
  const int nvec = (V - head) / N;
  const T* body = row + head;
  for (int v = tid; v < nvec; v += kNT) {
    float x[N];
    load16(body + (int64_t)v * N, x);
#pragma unroll
    for (int j = 0; j < N; ++j) f(head + v * N + j, x[j]);
  }
  const int t = head + nvec * N + tid;  // fewer than N elements left
  if (t < V) f(t, to_f(row[t]));
}

__device__ __forceinline__ float scaled(float x, float inv_t) {
  const float z = __fmul_rn(x, inv_t);  // never contracted into a later add: the host mirrors one multiply
  return z != z ? -INFINITY : z;
}

// 32-bit key with key(a) < key(b) <=> a < b (+0 and -0 share one key; no NaN reaches it)
__device__ __forceinline__ uint32_t zkey(float z) {
  if (z == 0.f) return 0x80000000u;
  const uint32_t b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ u64 mass_of(float z, float zmax, float scale) {
  if (z == zmax) return (u64)scale;  // also the +inf maximum, where z - zmax is NaN
  const float d = z - zmax;          // < 0
  if (d < -28.f) return 0;           // e < 2^-40 (ln 2^-40 = -27.73): truncates to 0 at every scale
  return (u64)(expf(d) * scale);
}

__device__ __forceinline__ Best block_best(Best b, Shared& sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float s = __shfl_xor(b.s, o, kWave);
    const int i = __shfl_xor(b.i, o, kWave);
    best_take(b, s, i);
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh.red_s[w] = b.s, sh.red_i[w] = b.i;
  __syncthreads();
  Best r{-INFINITY, INT_MAX};
#pragma unroll
  for (int k = 0; k < kWaves; ++k) best_take(r, sh.red_s[k], sh.red_i[k]);
  __syncthreads();
  return r;
}

// Scan sh.hist from the top bin down. With above(d) = base + sum of the bins over d and
// incl(d) = above(d) + hist[d], finds the one bin with above(d) < target <= incl(d) (compared in
// double; both sides are monotone in d). p_of_total >= 0: the target is p_of_total * (base + the
// sum of all bins), returned through `target`. Results in sh.sel_*; every thread returns after the
// barrier that publishes them.
__device__ __forceinline__ void select_bin(Shared& sh, u64 base, double p_of_total, double& target) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int hi = kBins - 1 - 2 * tid;
  const u64 a = sh.hist[hi], b = sh.hist[hi - 1];
  u64 inc = a + b;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const u64 up = __shfl_up(inc, o, kWave);
    if (l >= o) inc += up;
  }
  if (l == kWave - 1) sh.wtot[w] = inc;
  if (tid == 0) sh.sel_bin = -1, sh.sel_exact = 0, sh.sel_above = 0;
  __syncthreads();
  u64 before = base, total = base;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const u64 t = sh.wtot[k];
    if (k < w) before += t;
    total += t;
  }
  if (p_of_total >= 0.0) target = p_of_total * (double)total;
  const u64 above_hi = before + (inc - (a + b)), incl_hi = above_hi + a, incl_lo = incl_hi + b;
  if ((double)above_hi < target && target <= (double)incl_hi) {
    sh.sel_bin = hi, sh.sel_above = above_hi, sh.sel_exact = (double)incl_hi == target;
  } else if ((double)incl_hi < target && target <= (double)incl_lo) {
    sh.sel_bin = hi - 1, sh.sel_above = incl_hi, sh.sel_exact = (double)incl_lo == target;
  }
  __syncthreads();
}

// Radix select: the smallest key v >= floor_key with above(v) < target, where above(v) is the
// count (MASS = false) or the fixed-point mass (MASS = true) of the elements with key > v among
// those with key >= floor_key. MASS: target = top_p * (mass of all of them).
template <typename T, bool MASS>
__device__ __forceinline__ uint32_t radix_select(const T* __restrict__ row, int V, float inv_t, float zmax, float scale,
                                                 uint32_t floor_key, double target, double top_p, Shared& sh) {
  constexpr int kShift[3] = {21, 10, 0};
  constexpr int kPrefixShift[3] = {32, 21, 10};
  constexpr uint32_t kMask[3] = {0x7ffu, 0x7ffu, 0x3ffu};
  u64 base = 0;
  uint32_t prefix = 0;
#pragma unroll
  for (int lv = 0; lv < 3; ++lv) {
    for (int i = threadIdx.x; i < kBins; i += kNT) sh.hist[i] = 0;
    __syncthreads();
    for_row(row, V, [&](int, float x) {
      const float z = scaled(x, inv_t);
      const uint32_t key = zkey(z);
      if (key < floor_key || (uint32_t)((u64)key >> kPrefixShift[lv]) != prefix) return;
      const u64 v = MASS ? mass_of(z, zmax, scale) : 1ull;
      if (v) atomicAdd(&sh.hist[(key >> kShift[lv]) & kMask[lv]], v);
    });
    __syncthreads();
    select_bin(sh, base, MASS && lv == 0 ? top_p : -1.0, target);
    const int bin = sh.sel_bin;
    const u64 above = sh.sel_above;
    const int exact = sh.sel_exact;
    __syncthreads();  // sel_* read before the next select_bin resets them
    // no bin crossed the target (it exceeds the total): everything under this prefix is kept
    if (bin < 0) return max(floor_key, (uint32_t)((u64)prefix << kPrefixShift[lv]));
    prefix = lv == 2 ? (prefix << 10) | (uint32_t)bin : (prefix << 11) | (uint32_t)bin;
    base = above;
    if (exact) return max(floor_key, prefix << kShift[lv]);
  }
  return max(floor_key, prefix);
}

template <typename T>
__global__ __launch_bounds__(kNT) void sample_kernel(const T* __restrict__ logits, SampleArgs a) {
  __shared__ Shared sh;
  const int row_id = blockIdx.x;
  const int V = a.V;
  const T* row = logits + (int64_t)row_id * a.ld;
  Best best{-INFINITY, INT_MAX};
  if (!a.do_sample) {
    for_row(row, V, [&](int i, float x) { best_take(best, x, i); });
  } else {
    const float inv_t = a.inv_t;
    uint32_t tau = 0;
    float zmax = -INFINITY;
    bool live = true;
    if (a.top_p < 1.0) {  // only the masses need the maximum
      float m = -INFINITY;
      for_row(row, V, [&](int, float x) { m = fmaxf(m, scaled(x, inv_t)); });
      zmax = block_max<kNT>(m, sh.red_s);
      live = zmax > -INFINITY;  // nothing finite: nothing is kept, index 0 comes back
    }
    if (live && a.top_k > 0 && a.top_k < V)
      tau = radix_select<T, false>(row, V, inv_t, 0.f, 0.f, 0u, (double)a.top_k, 1.0, sh);
    if (live && a.top_p < 1.0)
      tau = radix_select<T, true>(row, V, inv_t, zmax, a.mass_scale, tau, 0.0, a.top_p, sh);
    // candidate mode: the rows are consecutive tokens of ONE sequence, so row t draws what the
    // one-row call draws at counter + t (noise row 0)
    const u64 ctr = (a.counter ? (u64)a.counter[0] : 0ull) + (a.candidates ? (u64)row_id : 0ull);
    const u64 nkey = hash_u64(hash_u64((u64)a.seed) + ctr);
    const u64 rbits = a.candidates ? 0ull : (u64)(uint32_t)row_id << 32;
    uint8_t* mask = a.keep_mask ? a.keep_mask + (int64_t)row_id * V : nullptr;
    for_row(row, V, [&](int i, float x) {
      const float z = scaled(x, inv_t);
      const bool keep = live && zkey(z) >= tau && z > -INFINITY;
      if (mask) mask[i] = keep;
      if (!keep) return;
      const uint32_t n = (uint32_t)(hash_u64(nkey ^ (rbits | (uint32_t)i)) >> 41);
      const float u = ((float)n + 0.5f) * 0x1p-23f;
      best_take(best, __fadd_rn(z, -logf(-logf(u))), i);
    });
  }
  best = block_best(best, sh);
  if (threadIdx.x != 0) return;
  const int64_t winner = best.i == INT_MAX ? 0 : best.i;  // all NaN / nothing kept
  int64_t tok = winner;
  if (a.finished) {
    const bool fin = a.finished[row_id] != 0;
    const int64_t n = a.step[0];
    if (fin && a.has_pad) tok = a.pad_id;
    if (!fin) {
      bool is_eos = false;
      for (int e = 0; e < a.n_eos; ++e) is_eos |= a.eos[e] == winner;
      if (is_eos) a.finished[row_id] = 1, a.finish_step[row_id] = n;
    }
    if (n >= 0 && n < a.out_cols) a.out[(int64_t)row_id * a.out_ld + n] = tok;
  }
  a.tokens[row_id] = tok;
}

}  // namespace

void sample_logits(const void* logits, DType dt, const SampleArgs& a, hipStream_t s) {
  if (dt == DType::BF16)
    hipLaunchKernelGGL(sample_kernel<bf16>, dim3(a.B), dim3(kNT), 0, s, (const bf16*)logits, a);
  else
    hipLaunchKernelGGL(sample_kernel<float>, dim3(a.B), dim3(kNT), 0, s, (const float*)logits, a);
  GRT_CHECK_LAUNCH();
}

}  // namespace grt
