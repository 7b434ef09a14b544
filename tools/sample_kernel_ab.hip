// A/B timing of the sampler kernel (csrc/kernels/sample.hip) against another revision of it, with and
// without the logits processors: bf16 logits [B, 128256], B = 1 and 8, device events around 200
// back-to-back launches, one warm-up round and 7 rounds in which every configuration runs once, so the two
// revisions alternate inside a round. Prints the median, smallest and largest round per configuration.
// Build (from the repository root; OLD is the revision to compare with, e.g. HEAD~1):
//   git show OLD:gke_ray_train_amd/csrc/kernels/sample.hip > /tmp/sample_old.hip
//   F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -Igke_ray_train_amd/csrc/include"
//   hipcc $F -Dsample_logits=sample_logits_parent -c /tmp/sample_old.hip -o /tmp/sample_old.o
//   hipcc $F -c gke_ray_train_amd/csrc/kernels/sample.hip -o /tmp/sample_new.o
//   hipcc $F -c tools/sample_kernel_ab.hip -o /tmp/ab.o
//   hipcc --offload-arch=gfx950 /tmp/ab.o /tmp/sample_new.o /tmp/sample_old.o -o /tmp/sample_kernel_ab
// The old revision is compiled against this tree's headers: fields of SampleArgs it does not know are ignored.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {
void sample_logits_parent(const void* logits, DType dt, const SampleArgs& a, hipStream_t s);
}
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct Cfg { const char* name; bool parent, sample; int top_k; double top_p; bool pen, minp; };

int main() {
  const int V = 128256, iters = 200, rounds = 7;
  const Cfg cfgs[] = {
      {"greedy parent", true, false, 0, 1.0, false, false},   {"greedy off", false, false, 0, 1.0, false, false},
      {"greedy penalty", false, false, 0, 1.0, true, false},  {"temp parent", true, true, 0, 1.0, false, false},
      {"temp off", false, true, 0, 1.0, false, false},        {"temp penalty", false, true, 0, 1.0, true, false},
      {"temp min_p", false, true, 0, 1.0, false, true},       {"k50p0.9 parent", true, true, 50, 0.9, false, false},
      {"k50p0.9 off", false, true, 50, 0.9, false, false},    {"k50p0.9 penalty", false, true, 50, 0.9, true, false},
      {"k50p0.9 min_p", false, true, 50, 0.9, false, true},   {"k50 off", false, true, 50, 1.0, false, false},
      {"k50 min_p", false, true, 50, 1.0, false, true}};
  const int NC = sizeof(cfgs) / sizeof(cfgs[0]);
  for (int B : {1, 8}) {
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 4.f);
    std::vector<uint16_t> h((size_t)B * V);
    for (auto& x : h) { float f = nd(rng); uint32_t u; memcpy(&u, &f, 4); x = (uint16_t)(u >> 16); }
    void* logits; int64_t* tokens; uint32_t* seen;
    const int64_t W = grt::seen_words(V);
    CK(hipMalloc(&logits, h.size() * 2)); CK(hipMalloc(&tokens, B * 8)); CK(hipMalloc(&seen, B * W * 4));
    CK(hipMemcpy(logits, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    std::vector<uint32_t> hs((size_t)B * W);
    for (auto& w : hs) w = rng() & rng() & rng();  // about 1 bit in 8
    CK(hipMemcpy(seen, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<std::vector<float>> us(NC);
    for (int r = -1; r < rounds; ++r)  // round -1 warms up
      for (int c = 0; c < NC; ++c) {
        const Cfg& k = cfgs[c];
        grt::SampleArgs a{};
        a.B = B, a.V = V, a.ld = V, a.do_sample = k.sample, a.inv_t = 1.f / 0.8f, a.top_k = k.top_k, a.top_p = k.top_p;
        a.mass_scale = std::ldexp(1.0f, 40), a.seed = 1, a.tokens = tokens, a.penalty = 1.f;
        if (k.pen) a.seen = seen, a.seen_ld = W, a.penalty = 1.3f;
        if (k.minp) a.min_p_on = true, a.ln_min_p = (float)std::log(0.05);
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i)
          (k.parent ? grt::sample_logits_parent : grt::sample_logits)(logits, grt::DType::BF16, a, 0);
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us[c].push_back(ms * 1000.f / iters);
      }
    for (int c = 0; c < NC; ++c) {
      std::sort(us[c].begin(), us[c].end());
      printf("B=%d %-16s median %7.2f us  min %7.2f  max %7.2f\n", B, cfgs[c].name, us[c][rounds / 2], us[c][0], us[c][rounds - 1]);
    }
    CK(hipFree(logits)); CK(hipFree(tokens)); CK(hipFree(seen));
  }
  return 0;
}
