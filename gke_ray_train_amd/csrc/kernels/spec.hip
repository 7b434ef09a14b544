// Accept and draft steps of prompt-lookup speculative decoding, one launch of one workgroup at the
// end of the captured verify step (batch 1). ops/_ref.py::spec_accept and ::prompt_lookup_draft are
// the host implementations; all of it is integer work, so the results are the same bit for bit.
//
// The verify step ran the tokens ids[0 .. K] = [x0, d_1 .. d_K] at positions pos[0 .. K] and the
// sampler's candidate mode left cand[t], the token drawn from logits row t (token number n + t,
// n = n_step[0] tokens emitted so far). Thread 0 accepts: a = the longest prefix with drafts[i] ==
// cand[i]; cand[0 .. a] go to out[n ...] and to the history hist[prompt_len + n ...], cut after the
// first EOS and at max_new; n_step and counter move on by the number emitted (e), so do pos[t] and
// lens[0] (the cache slots of rejected drafts lie past the new valid length and are rewritten by
// the next step). A row that is finished or full is inert: no state changes. Then the whole
// workgroup drafts for the next step: plan[n' .. n' + K) when a plan is given (test hook), else the
// prompt lookup over the n_hist = prompt_len + n' history tokens: for ngram = min(N, n_hist - 1)
// down to 1 every thread scans start positions s = tid, tid + 256, ... for hist[s .. s + ngram) ==
// the last ngram tokens with s + ngram < n_hist, the block takes the largest s, and the first
// ngram with a match gives drafts hist[s + ngram ...] cut at n_hist; open slots are -1. ids[0] is
// the last emitted token and ids[1 + i] the draft, or 0 where the draft is no valid token id (the
// embedding must read a real row; such a draft is never accepted because `drafts` keeps the -1).
// One launch rather than two: the accept is a few dozen scalar operations, and the lookup needs
// its result (the new history length), so a second launch would only add its latency.
#include <hip/hip_runtime.h>

#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
namespace {

constexpr int kSpecThreads = 256;

__global__ __launch_bounds__(kSpecThreads) void spec_advance_kernel(SpecAdvanceArgs a) {
  __shared__ int64_t sh_n;     // tokens emitted after this step
  __shared__ int sh_inert;
  __shared__ int sh_best[kSpecThreads / 64];
  const int tid = threadIdx.x;
  const int K = a.K;
  if (tid == 0) {
    const int64_t n = a.n_step[0];
    const bool inert = a.finished[0] != 0 || n >= a.max_new;
    int64_t e = 0;
    if (!inert) {
      int acc = 0;
      while (acc < K && a.drafts[acc] == a.cand[acc]) ++acc;
      bool fin = false;
      int64_t last = 0;
      for (int i = 0; i <= acc && !fin && n + e < a.max_new; ++i) {
        last = a.cand[i];
        a.out[n + e] = last;
        a.hist[a.prompt_len + n + e] = last;
        ++e;
        for (int q = 0; q < a.n_eos; ++q) fin |= a.eos[q] == last;
      }
      if (fin) a.finished[0] = 1, a.finish_step[0] = n + e - 1;
      a.ids[0] = last;
      a.n_step[0] = n + e;
      a.counter[0] += e;
      for (int t = 0; t <= K; ++t) a.pos[t] += (int32_t)e;
      a.lens[0] += (int32_t)e;
      a.done[0] = fin || n + e >= a.max_new;
    }
    sh_n = n + e;
    sh_inert = inert;
  }
  __syncthreads();  // also orders thread 0's history writes before the block's reads
  if (sh_inert) return;
  const int64_t n = sh_n;
  if (a.plan) {
    if (tid < K) {
      const int64_t i = n + tid;
      const int64_t d = i < a.plan_len ? a.plan[i] : -1;
      a.drafts[tid] = d;
      a.ids[1 + tid] = d >= 0 && d < a.vocab ? d : 0;
    }
    return;
  }
  const int64_t nh = a.prompt_len + n;
  int64_t start = -1;  // first token of the continuation
  for (int ng = nh - 1 < a.N ? (int)(nh - 1) : a.N; ng >= 1; --ng) {
    int best = -1;
    for (int64_t s = tid; s + ng < nh; s += kSpecThreads) {
      bool eq = true;
      for (int i = 0; i < ng && eq; ++i) eq = a.hist[s + i] == a.hist[nh - ng + i];
      if (eq) best = (int)s;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    __syncthreads();  // the previous round's sh_best has been read
    if ((tid & 63) == 0) sh_best[tid >> 6] = best;
    __syncthreads();
    best = sh_best[0];
#pragma unroll
    for (int w = 1; w < kSpecThreads / 64; ++w) best = max(best, sh_best[w]);
    if (best >= 0) {
      start = best + ng;
      break;  // uniform: every thread read the same sh_best
    }
  }
  if (tid < K) {
    const int64_t i = start + tid;
    const int64_t d = start >= 0 && i < nh ? a.hist[i] : -1;
    a.drafts[tid] = d;
    a.ids[1 + tid] = d >= 0 && d < a.vocab ? d : 0;
  }
}

}  // namespace

void spec_advance(const SpecAdvanceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(spec_advance_kernel, dim3(1), dim3(kSpecThreads), 0, s, a);
  GRT_CHECK_LAUNCH();
}

}  // namespace grt
