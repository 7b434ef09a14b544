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
// Logits processors (HF's names; ops/_ref.py::sample_process / sample_filter are the definition):
//   min_new_tokens = m (state mode): while step[0] < m the eos ids count as -inf in every pass.
//   repetition_penalty = theta != 1 with the seen bitmap [B, W] (bit i & 31 of word i >> 5 of row b:
//   token i is in row b's prompt or was emitted): a seen token's logit x becomes x > 0 ? x / theta :
//   x * theta, one correctly rounded fp32 operation, before the 1 / T multiply; -inf stays -inf and
//   NaN still ends as -inf. Greedy is then the argmax of the processed logits. The thread that
//   writes the token also sets its bit (load, or, store: the workgroup owns the row), unless the
//   row was finished before this call.
//   min_p in (0, 1] (sampling): keeps i iff z_i >= z_max + ln(min_p), one fp32 add of the fp32
//   ln(min_p) the host computed and one compare; intersected with the top-k / top-p sets. It is one
//   more key threshold: it needs z_max, which comes from top-p's maximum pass, else from the first
//   pass of the top-k select, else (temperature only) from a maximum pass of its own.
//   All three are compile-time variants of the kernel (PEN, SUP, MINP): the passes of the plain
//   instantiations are the code they were without the processors.
//   Where the bitmap is read from (LDS or global memory) is part of PEN, so no pass branches on it.
//   seen_tokens_add fills the bitmap from the prompt ids (vector atomic OR, grid-stride).
//
// LDS: the 16 KB histogram plus, with PEN and V <= 262144, the row's W = ceil(V / 32) (rounded up to
// 4) bitmap words, copied once with 16-byte loads before the first pass (16 KB at V = 128256, 32 KB
// at the limit); every pass reads its bits there. Larger vocabularies read the words from global
// memory.
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
// (fewer when a bin boundary hits the target exactly). min_p adds one pass to temperature only and
// none to the others; the penalty and the suppression add none.
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
  float row_max;  // radix_select with track_max: the row's maximum z
};

// The row's seen bitmap (PEN, V <= kSeenLdsMaxV): dynamic LDS behind the static Shared block.
extern __shared__ uint4 seen_lds[];

// Suppression, then the repetition penalty, of logit x at index i. PEN: 0 off, 1 the row's bitmap
// words are in seen_lds, 2 they are read from global memory.
template <int PEN, bool SUP>
struct Proc {
  const uint32_t* seen_g;   // PEN == 2
  float theta;              // PEN
  int sup[kSampleMaxEos];   // SUP: the ids that count as -inf now (-1: none)
  __device__ __forceinline__ float operator()(int i, float x) const {
    if constexpr (SUP) {
#pragma unroll
      for (int e = 0; e < kSampleMaxEos; ++e)
        if (i == sup[e]) x = -INFINITY;
    }
    if constexpr (PEN != 0) {
      const uint32_t w = PEN == 2 ? seen_g[i >> 5] : reinterpret_cast<const uint32_t*>(seen_lds)[i >> 5];
      if ((w >> (i & 31)) & 1u) x = x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta);
    }
    return x;
  }
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
// those with key >= floor_key. MASS: target = top_p * (mass of all of them). TRACK and track_max: the
// first pass also takes the row's maximum z, left in sh.row_max (min_p without top-p).
template <typename T, bool MASS, bool TRACK, typename P>
__device__ __forceinline__ uint32_t radix_select(const T* __restrict__ row, int V, const P& proc, float inv_t,
                                                 float zmax, float scale, uint32_t floor_key, double target,
                                                 double top_p, Shared& sh, bool track_max = false) {
  constexpr int kShift[3] = {21, 10, 0};
  constexpr int kPrefixShift[3] = {32, 21, 10};
  constexpr uint32_t kMask[3] = {0x7ffu, 0x7ffu, 0x3ffu};
  u64 base = 0;
  uint32_t prefix = 0;
#pragma unroll
  for (int lv = 0; lv < 3; ++lv) {
    for (int i = threadIdx.x; i < kBins; i += kNT) sh.hist[i] = 0;
    __syncthreads();
    float m = -INFINITY;
    for_row(row, V, [&](int i, float x) {
      const float z = scaled(proc(i, x), inv_t);
      if constexpr (TRACK) {
        if (track_max) m = fmaxf(m, z);
      }
      const uint32_t key = zkey(z);
      if (key < floor_key || (uint32_t)((u64)key >> kPrefixShift[lv]) != prefix) return;
      const u64 v = MASS ? mass_of(z, zmax, scale) : 1ull;
      if (v) atomicAdd(&sh.hist[(key >> kShift[lv]) & kMask[lv]], v);
    });
    __syncthreads();
    if constexpr (TRACK) {
      if (lv == 0 && track_max) {
        m = block_max<kNT>(m, sh.red_s);
        if (threadIdx.x == 0) sh.row_max = m;  // published by select_bin's barriers
      }
    }
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

template <typename T, int PEN, bool SUP, bool MINP>
__global__ __launch_bounds__(kNT) void sample_kernel(const T* __restrict__ logits, SampleArgs a) {
  __shared__ Shared sh;
  const int row_id = blockIdx.x;
  const int V = a.V;
  const T* row = logits + (int64_t)row_id * a.ld;
  Proc<PEN, SUP> proc;
  if constexpr (SUP) {
    const bool on = a.step[0] < a.min_new;
#pragma unroll
    for (int e = 0; e < kSampleMaxEos; ++e)
      proc.sup[e] = on && e < a.n_eos && a.eos[e] >= 0 && a.eos[e] < V ? (int)a.eos[e] : -1;
  }
  uint32_t* seen_row = nullptr;
  if constexpr (PEN != 0) {
    seen_row = a.seen + (int64_t)row_id * a.seen_ld;
    proc.theta = a.penalty;
    proc.seen_g = seen_row;
  }
  if constexpr (PEN == 1) {  // rows are 16-byte aligned and a multiple of 4 words long
    const int nvec = (int)(seen_words(V) / 4);
    for (int v = threadIdx.x; v < nvec; v += kNT) seen_lds[v] = reinterpret_cast<const uint4*>(seen_row)[v];
    __syncthreads();
  }
  Best best{-INFINITY, INT_MAX};
  if (!a.do_sample) {
    for_row(row, V, [&](int i, float x) { best_take(best, proc(i, x), i); });
  } else {
    const float inv_t = a.inv_t;
    uint32_t tau = 0;
    float zmax = -INFINITY;
    bool live = true;
    if (a.top_p < 1.0) {  // only the masses need the maximum
      float m = -INFINITY;
      for_row(row, V, [&](int i, float x) { m = fmaxf(m, scaled(proc(i, x), inv_t)); });
      zmax = block_max<kNT>(m, sh.red_s);
      live = zmax > -INFINITY;  // nothing finite: nothing is kept, index 0 comes back
    }
    const bool topk = a.top_k > 0 && a.top_k < V;
    // min_p needs the maximum too: without top-p the first pass of the top-k select takes it along,
    // and temperature alone pays a pass for it
    bool take_max = false;
    if constexpr (MINP) {
      take_max = !(a.top_p < 1.0);
      if (take_max && !topk) {
        float m = -INFINITY;
        for_row(row, V, [&](int i, float x) { m = fmaxf(m, scaled(proc(i, x), inv_t)); });
        zmax = block_max<kNT>(m, sh.red_s);
      }
    }
    if (live && topk)
      tau = radix_select<T, false, MINP>(row, V, proc, inv_t, 0.f, 0.f, 0u, (double)a.top_k, 1.0, sh, take_max);
    if constexpr (MINP) {
      if (take_max && topk) zmax = sh.row_max;
      if (take_max) live = zmax > -INFINITY;
    }
    if (live && a.top_p < 1.0)
      tau = radix_select<T, true, false>(row, V, proc, inv_t, zmax, a.mass_scale, tau, 0.0, a.top_p, sh);
    if constexpr (MINP) {
      if (live) tau = max(tau, zkey(__fadd_rn(zmax, a.ln_min_p)));  // z >= z_max + ln(min_p)
    }
    // candidate mode: the rows are consecutive tokens of ONE sequence, so row t draws what the
    // one-row call draws at counter + t (noise row 0)
    const u64 ctr = (a.counter ? (u64)a.counter[0] : 0ull) + (a.candidates ? (u64)row_id : 0ull);
    const u64 nkey = hash_u64(hash_u64((u64)a.seed) + ctr);
    const u64 rbits = a.candidates ? 0ull : (u64)(uint32_t)row_id << 32;
    uint8_t* mask = a.keep_mask ? a.keep_mask + (int64_t)row_id * V : nullptr;
    for_row(row, V, [&](int i, float x) {
      const float z = scaled(proc(i, x), inv_t);
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
  bool fin = false;
  if (a.finished) {
    fin = a.finished[row_id] != 0;
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
  if constexpr (PEN != 0) {
    if (!fin) seen_row[winner >> 5] |= 1u << (winner & 31);  // every pass over the row is behind block_best's barriers
  }
}

// One thread per id, grid-stride. lens: row b contributes ids[b][0 .. lens[b]).
__global__ __launch_bounds__(256) void seen_add_kernel(const int64_t* __restrict__ ids, int64_t ids_ld,
                                                       const int32_t* __restrict__ lens, int64_t S, int64_t n,
                                                       int64_t V, uint32_t* __restrict__ seen, int64_t seen_ld) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t b = e / S, s = e - b * S;
    if (lens && s >= lens[b]) continue;
    const int64_t id = ids[b * ids_ld + s];
    if (id < 0 || id >= V) continue;
    atomicOr(&seen[b * seen_ld + (id >> 5)], 1u << (id & 31));
  }
}

template <typename T, int PEN, bool SUP>
auto kernel_minp(bool minp) {
  return minp ? sample_kernel<T, PEN, SUP, true> : sample_kernel<T, PEN, SUP, false>;
}
template <typename T, int PEN>
auto kernel_sup(bool sup, bool minp) {
  return sup ? kernel_minp<T, PEN, true>(minp) : kernel_minp<T, PEN, false>(minp);
}

template <typename T>
void launch_sample(const T* logits, const SampleArgs& a, hipStream_t s) {
  const int pen = a.seen == nullptr ? 0 : a.V <= kSeenLdsMaxV ? 1 : 2;
  const bool sup = a.min_new > 0 && a.n_eos > 0, minp = a.do_sample && a.min_p_on;
  const size_t lds = pen == 1 ? (size_t)seen_words(a.V) * sizeof(uint32_t) : 0;
  auto k = pen == 0 ? kernel_sup<T, 0>(sup, minp) : pen == 1 ? kernel_sup<T, 1>(sup, minp) : kernel_sup<T, 2>(sup, minp);
  hipLaunchKernelGGL(k, dim3(a.B), dim3(kNT), lds, s, logits, a);
}

}  // namespace

void sample_logits(const void* logits, DType dt, const SampleArgs& a, hipStream_t s) {
  if (dt == DType::BF16)
    launch_sample((const bf16*)logits, a, s);
  else
    launch_sample((const float*)logits, a, s);
  GRT_CHECK_LAUNCH();
}

constexpr int kSeenAddMaxBlocks = 256;

void seen_tokens_add(const int64_t* ids, int64_t ids_ld, const int32_t* lens, int B, int64_t S, int64_t V,
                     uint32_t* seen, int64_t seen_ld, hipStream_t s) {
  const int64_t n = (int64_t)B * S;
  if (n == 0) return;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, kSeenAddMaxBlocks);
  hipLaunchKernelGGL(seen_add_kernel, dim3(blocks), dim3(256), 0, s, ids, ids_ld, lens, S, n, V, seen, seen_ld);
  GRT_CHECK_LAUNCH();
}

}  // namespace grt
