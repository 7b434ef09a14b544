// AdamW with 8-bit block-quantised moments for gfx950 (the bitsandbytes "8-bit optimizer" role:
// OPTIM=paged_adamw_8bit / adamw_8bit / adamw_bnb_8bit), plus the two standalone
// quantise / dequantise kernels that state-dict loading and saving use.
//
// Scheme (defined on the host in ops/_ref.py; the tables below come from the same formula, evaluated
// in double at compile time): a block is 256 consecutive elements of the flat state, with one fp32
// absmax; an element is the uint8 code of the table entry nearest to x / absmax; the dequantised
// value is fp32(table[code] * absmax). Two 256-entry "dynamic" tables (decades 10^-6 .. 10^0, a linear
// fraction per decade, twice the fraction steps per higher decade): signed for exp_avg, unsigned for
// exp_avg_sq. Both hold 0 and +-1 / 1, so requantising a dequantised block gives its codes back.
//
// One pass over HBM per step: 10 bytes per element (p 2+2, g 2, codes 1+1 and 1+1) plus 16 bytes per
// 256 elements, against 22 with fp32 moments. A lane holds 8 consecutive elements, so 32 lanes hold a
// block and the new absmax is a half-wave shuffle reduction: no LDS traffic and no barrier between
// the update and the quantisation, which runs from registers. LDS holds only the tables (13 KiB).
// The code of x is the number of table midpoints below it (the same count the host's bucketize gives,
// so ties and entries cannot disagree), found by a cell lookup and one compare: see q8_code.
#include "grt_adam.h"
#include "grt_common.h"
#include "grt_kernels.h"

namespace grt {

bool adamw_fastmath();  // optim.hip: GRT_ADAMW_FASTMATH=0 selects the IEEE arithmetic

namespace {

constexpr int kNT = 256;
constexpr int kQB = 256;                 // elements per quantisation block
constexpr int kE = 8;                    // elements per lane
constexpr int kChunk = kNT * kE;         // elements per workgroup and iteration: eight blocks
constexpr int kZeroS = 127, kZeroU = 0;  // codes of 0.0

// Finding the code of x: the number of table midpoints below it. The bits of |x| above the low 16
// (exponent and 7 mantissa bits) name a cell [lo, hi) of relative width 1/128, narrower than any gap of
// the tables, so a cell holds at most kQ8Probe midpoints. A byte table gives the number of midpoints
// below the cell (for a negative x: up to -hi), and kQ8Probe compares against the midpoints themselves
// finish the count (a static_assert below checks the tables against kQ8Probe): one byte and one dword
// from LDS and ~8 VALU per code, against eight dependent
// bisection steps (8 LDS reads, ~30 VALU). Cells start at 2^-24, below the smallest midpoint (1.6e-7).
constexpr int kQ8Base = (127 - 24) << 7;  // (bits of 2^-24) >> 16
constexpr int kQ8Cells = 24 * 128 + 1;    // up to and including the cell of 1.0
constexpr int kQ8Probe = 1;

// tab[0]: signed entries, tab[1]: unsigned entries; mid[0] / mid[1]: their 255 midpoints, then +inf;
// lut_u: unsigned starts per cell; lut_s: signed starts, the cells of x >= 0 first, then those of x < 0
struct Q8Tables {
  float tab[2][256];
  float mid[2][256 + kQ8Probe];
  uint8_t lut_u[kQ8Cells];
  uint8_t lut_s[2 * kQ8Cells];
  uint8_t pad[16 - (3 * kQ8Cells) % 16];
  int max_in_cell;
};

constexpr float q8_cell_lo(int c) { return c <= 0 ? 0.f : __builtin_bit_cast(float, (uint32_t)(c + kQ8Base) << 16); }

constexpr Q8Tables make_q8_tables() {
  Q8Tables t{};
  constexpr double decade[7] = {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0};
  for (int u = 0; u < 2; ++u) {  // u = 0: one fraction step in the lowest decade (signed); 1: two
    double mag[254] = {};
    int nm = 0;
    for (int i = 0; i < 7; ++i) {
      const int k = (u + 1) << i;
      for (int j = 0; j < k; ++j) mag[nm++] = decade[i] * (0.1 + 0.9 * (j + 0.5) / (double)k);
    }
    int c = 0;
    if (u == 0) {  // -1, the magnitudes mirrored without the smallest one, 0, the magnitudes, 1
      t.tab[0][c++] = -1.f;
      for (int j = nm - 1; j >= 1; --j) t.tab[0][c++] = (float)(-mag[j]);
    }
    t.tab[u][c++] = 0.f;
    for (int j = 0; j < nm; ++j) t.tab[u][c++] = (float)mag[j];
    t.tab[u][c++] = 1.f;
    for (int j = 0; j < 255; ++j) t.mid[u][j] = (float)(((double)t.tab[u][j] + (double)t.tab[u][j + 1]) / 2);
    for (int j = 255; j < 256 + kQ8Probe; ++j) t.mid[u][j] = __builtin_huge_valf();
  }
  int worst = 0;
  // x >= 0 in cell c: the midpoints below lo count, those in [lo, hi) are probed
  for (int sg = 0; sg < 2; ++sg) {
    const float* mid = t.mid[sg ? 0 : 1];
    uint8_t* lut = sg ? t.lut_s : t.lut_u;
    int below = 0;
    for (int c = 0; c < kQ8Cells; ++c) {
      while (below < 255 && mid[below] < q8_cell_lo(c)) ++below;
      lut[c] = (uint8_t)below;
      int in = 0;
      while (below + in < 255 && mid[below + in] < q8_cell_lo(c + 1)) ++in;
      worst = in > worst ? in : worst;
    }
  }
  // x < 0, |x| in cell c, so x in (-hi, -lo]: the midpoints up to -hi count, those in (-hi, -lo) are probed
  int below = 0;
  for (int c = kQ8Cells - 1; c >= 0; --c) {
    while (below < 255 && t.mid[0][below] <= -q8_cell_lo(c + 1)) ++below;
    t.lut_s[kQ8Cells + c] = (uint8_t)below;
    int in = 0;
    while (below + in < 255 && t.mid[0][below + in] < -q8_cell_lo(c)) ++in;
    worst = in > worst ? in : worst;
  }
  t.max_in_cell = worst;
  return t;
}

__device__ const Q8Tables kQ8 = make_q8_tables();
static_assert(make_q8_tables().max_in_cell <= kQ8Probe, "a cell holds more midpoints than q8_code probes");
static_assert(sizeof(Q8Tables) % 4 == 0, "copied to LDS as dwords");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// the workgroup's copy of the tables
__device__ __forceinline__ void load_q8_tables(Q8Tables* lds) {
  for (int i = threadIdx.x; i < (int)(sizeof(Q8Tables) / 4); i += kNT)
    reinterpret_cast<uint32_t*>(lds)[i] = reinterpret_cast<const uint32_t*>(&kQ8)[i];
  __syncthreads();
}

// number of midpoints below x (NaN: 0): the code of the entry nearest to x, the lower one at a tie
template <bool SIGNED>
__device__ __forceinline__ uint32_t q8_code(float x, const Q8Tables* t) {
  const uint32_t u = __float_as_uint(x);
  int cell = (int)((u & 0x7fffffffu) >> 16) - kQ8Base;
  cell = cell < 0 ? 0 : (cell > kQ8Cells - 1 ? kQ8Cells - 1 : cell);
  uint32_t c;
  if constexpr (SIGNED)
    c = t->lut_s[cell + (int)(u >> 31) * kQ8Cells];
  else
    c = t->lut_u[cell];
  const float* mid = t->mid[SIGNED ? 0 : 1] + c;
#pragma unroll
  for (int k = 0; k < kQ8Probe; ++k) c += x > mid[k] ? 1 : 0;
  return x != x ? 0 : c;
}

// max |x| over the 32 lanes that hold a block, on the bit patterns: unsigned order is the order of
// non-negative floats, and NaN sorts above infinity, so a non-finite element is never dropped
__device__ __forceinline__ uint32_t block_max_bits(uint32_t b) {
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)b, o, kWave);
    b = b > t ? b : t;
  }
  return b;
}

// x -> x / absmax as the quantiser sees it; 0 for an all-zero block
template <bool FAST>
struct Q8Norm {
  float inv, a;
  __device__ __forceinline__ explicit Q8Norm(float absmax) : a(absmax) {
    inv = absmax == 0.f ? 0.f : (FAST ? __builtin_amdgcn_rcpf(absmax) : 1.f);
  }
  __device__ __forceinline__ float operator()(float x) const {
    if constexpr (FAST) return x * inv;
    return a == 0.f ? 0.f : x / a;
  }
};

__device__ __forceinline__ u32x2 pack8(const uint32_t* c) {
  u32x2 r;
  r[0] = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  r[1] = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
  return r;
}

// T: bf16 (p and g; master optional) or float (p and g; no master). A16: p and g are 16-byte aligned
// (otherwise 8-byte aligned bf16 views, loaded as two 8-byte halves). The code arrays are 8-byte
// aligned, master 16-byte. ioff: flat element index of p[0] (a multiple of 256: the slice starts on
// a block boundary, so its blocks are the whole buffer's).
template <typename T, bool A16, bool FAST>
__global__ __launch_bounds__(kNT) void adamw8_kernel(T* __restrict__ p, const T* __restrict__ g,
                                                     uint8_t* __restrict__ cm, float* __restrict__ am,
                                                     uint8_t* __restrict__ cv, float* __restrict__ av,
                                                     float* __restrict__ master, int64_t n,
                                                     const float* __restrict__ hyper,
                                                     const float* __restrict__ gsp, uint64_t ioff) {
  __shared__ __attribute__((aligned(16))) Q8Tables lds;
  load_q8_tables(&lds);
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
  const float bc1 = hyper[5], bc2 = hyper[6];
  const float gs = hyper[7] * (gsp ? gsp[1] : 1.f);
  const float step = lr / bc1;
  const float rbc2 = rsqrtf(bc2);
  const float decay = 1.f - lr * wd;
  const bool sr = sizeof(T) == 2 && master == nullptr && hyper[8] != 0.f;
  const uint64_t srkey = hash_u64(0x5352ull ^ ((uint64_t)hyper[9] << 20));
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  // the trip count is uniform over the workgroup: every lane takes part in the shuffles
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t o = (c * kNT + threadIdx.x) * kE;
    const int cnt = o >= n ? 0 : (n - o >= kE ? kE : (int)(n - o));
    // lanes (and elements) past n hold zeros: they change no maximum and are never stored
    float pf[kE], gf[kE], m[kE], v[kE];
    uint32_t qm[kE], qv[kE];
    if (cnt == kE) {
      const u32x2 wm = *reinterpret_cast<const u32x2*>(cm + o), wv = *reinterpret_cast<const u32x2*>(cv + o);
#pragma unroll
      for (int k = 0; k < kE; ++k) {
        qm[k] = (wm[k >> 2] >> (8 * (k & 3))) & 0xffu;
        qv[k] = (wv[k >> 2] >> (8 * (k & 3))) & 0xffu;
      }
      if constexpr (sizeof(T) == 2) {
        bf16x8 tp, tg;
        if constexpr (A16) {
          tp = *reinterpret_cast<const bf16x8*>(p + o);
          tg = *reinterpret_cast<const bf16x8*>(g + o);
        } else {
          tp = __builtin_shufflevector(*reinterpret_cast<const bf16x4*>(p + o),
                                       *reinterpret_cast<const bf16x4*>(p + o + 4), 0, 1, 2, 3, 4, 5, 6, 7);
          tg = __builtin_shufflevector(*reinterpret_cast<const bf16x4*>(g + o),
                                       *reinterpret_cast<const bf16x4*>(g + o + 4), 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int k = 0; k < kE; ++k) {
          pf[k] = to_f(tp[k]);
          gf[k] = to_f(tg[k]) * gs;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 tp = *reinterpret_cast<const f32x4*>(p + o + 4 * q);
          const f32x4 tg = *reinterpret_cast<const f32x4*>(g + o + 4 * q);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            pf[4 * q + k] = tp[k];
            gf[4 * q + k] = tg[k] * gs;
          }
        }
      }
      if (master) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(master + o + 4 * q);
#pragma unroll
          for (int k = 0; k < 4; ++k) pf[4 * q + k] = t[k];
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kE; ++k) {
        const bool in = k < cnt;
        qm[k] = in ? cm[o + k] : kZeroS;
        qv[k] = in ? cv[o + k] : kZeroU;
        pf[k] = in ? (master ? master[o + k] : to_f(p[o + k])) : 0.f;
        gf[k] = in ? to_f(g[o + k]) * gs : 0.f;
      }
    }
    const float am0 = cnt ? am[o / kQB] : 0.f, av0 = cnt ? av[o / kQB] : 0.f;
    uint32_t mb = 0, vb = 0;
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      m[k] = lds.tab[0][qm[k]] * am0;
      v[k] = lds.tab[1][qv[k]] * av0;
      pf[k] = adam_elem<FAST>(pf[k], gf[k], m[k], v[k], b1, b2, rbc2, eps, decay, step);
      const uint32_t um = __float_as_uint(m[k]) & 0x7fffffffu, uv = __float_as_uint(v[k]) & 0x7fffffffu;
      mb = mb > um ? mb : um;
      vb = vb > uv ? vb : uv;
    }
    // the parameter (and the master copy) from the fp32 new moments
    if (cnt == kE) {
      if (master) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          f32x4 t;
#pragma unroll
          for (int k = 0; k < 4; ++k) t[k] = pf[4 * q + k];
          *reinterpret_cast<f32x4*>(master + o + 4 * q) = t;
        }
      }
      if constexpr (sizeof(T) == 2) {
        bf16x8 t;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (sr) {
            const uint64_t h = sr_bits4<FAST>(srkey, (ioff + (uint64_t)(o + 4 * q)) & ~3ull);
#pragma unroll
            for (int k = 0; k < 4; ++k) t[4 * q + k] = sr_bf16(pf[4 * q + k], (uint32_t)(h >> (16 * k)) & 0xffffu);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) t[4 * q + k] = from_f<bf16>(pf[4 * q + k]);
          }
        }
        if constexpr (A16) {
          *reinterpret_cast<bf16x8*>(p + o) = t;
        } else {
          *reinterpret_cast<bf16x4*>(p + o) = __builtin_shufflevector(t, t, 0, 1, 2, 3);
          *reinterpret_cast<bf16x4*>(p + o + 4) = __builtin_shufflevector(t, t, 4, 5, 6, 7);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          f32x4 t;
#pragma unroll
          for (int k = 0; k < 4; ++k) t[k] = pf[4 * q + k];
          *reinterpret_cast<f32x4*>(p + o + 4 * q) = t;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kE; ++k) {  // (unrolled and guarded: pf stays in registers)
        if (k >= cnt) break;
        const int64_t j = o + k;
        if (master) master[j] = pf[k];
        if constexpr (sizeof(T) == 2) {
          const uint64_t fi = ioff + (uint64_t)j;
          p[j] = sr ? sr_bf16(pf[k], (uint32_t)(sr_bits4<FAST>(srkey, fi & ~3ull) >> (16 * (fi & 3))) & 0xffffu)
                    : from_f<bf16>(pf[k]);
        } else {
          p[j] = pf[k];
        }
      }
    }
    // the block's new absmax over its 32 lanes, then the codes from registers
    const float am1 = __uint_as_float(block_max_bits(mb)), av1 = __uint_as_float(block_max_bits(vb));
    const Q8Norm<FAST> nm(am1), nv(av1);
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      qm[k] = q8_code<true>(nm(m[k]), &lds);
      qv[k] = q8_code<false>(nv(v[k]), &lds);
    }
    if (cnt == kE) {
      *reinterpret_cast<u32x2*>(cm + o) = pack8(qm);
      *reinterpret_cast<u32x2*>(cv + o) = pack8(qv);
    } else {
#pragma unroll
      for (int k = 0; k < kE; ++k)
        if (k < cnt) {
          cm[o + k] = (uint8_t)qm[k];
          cv[o + k] = (uint8_t)qv[k];
        }
    }
    if (cnt && (threadIdx.x & 31) == 0) {
      am[o / kQB] = am1;
      av[o / kQB] = av1;
    }
  }
}

// fp32 x [n] -> codes [n], absmax [ceil(n / 256)]; IEEE division, as on the host
template <bool SIGNED>
__global__ __launch_bounds__(kNT) void quantize8_kernel(const float* __restrict__ x, uint8_t* __restrict__ codes,
                                                        float* __restrict__ absmax, int64_t n) {
  __shared__ __attribute__((aligned(16))) Q8Tables lds;
  load_q8_tables(&lds);
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t o = (c * kNT + threadIdx.x) * kE;
    const int cnt = o >= n ? 0 : (n - o >= kE ? kE : (int)(n - o));
    float xv[kE];
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      xv[k] = k < cnt ? x[o + k] : 0.f;
      const uint32_t u = __float_as_uint(xv[k]) & 0x7fffffffu;
      b = b > u ? b : u;
    }
    const float a = __uint_as_float(block_max_bits(b));
    const Q8Norm<false> nx(a);
#pragma unroll
    for (int k = 0; k < kE; ++k)
      if (k < cnt) codes[o + k] = (uint8_t)q8_code<SIGNED>(nx(xv[k]), &lds);
    if (cnt && (threadIdx.x & 31) == 0) absmax[o / kQB] = a;
  }
}

template <bool SIGNED>
__global__ __launch_bounds__(kNT) void dequantize8_kernel(const uint8_t* __restrict__ codes,
                                                          const float* __restrict__ absmax, float* __restrict__ out,
                                                          int64_t n) {
  __shared__ __attribute__((aligned(16))) Q8Tables lds;
  load_q8_tables(&lds);
  for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT)
    out[i] = lds.tab[SIGNED ? 0 : 1][codes[i]] * absmax[i / kQB];
}

unsigned q8_grid(int64_t n, int per_block, int max_blocks) {
  int64_t nb = (n + per_block - 1) / per_block;
  // every workgroup first copies the tables (13 KiB) to LDS, so fewer and longer-lived workgroups than
  // the fp32 kernel's 16384: 2^27 bf16 elements took 335 us at 16384, 327 at 1280, 316 at 4096
  // (profiles/adamw8.md)
  if (nb > 4096) nb = 4096;
  if (max_blocks > 0 && nb > max_blocks) nb = max_blocks;
  return (unsigned)(nb < 1 ? 1 : nb);
}

template <typename T, bool FAST>
void launch_adamw8(dim3 grid, hipStream_t s, T* p, const T* g, uint8_t* cm, float* am, uint8_t* cv, float* av,
                   float* master, int64_t n, const float* hyper, const float* gsp, uint64_t ioff) {
  const bool a16 = reinterpret_cast<uintptr_t>(p) % 16 == 0 && reinterpret_cast<uintptr_t>(g) % 16 == 0;
  if (a16 || sizeof(T) == 4)
    hipLaunchKernelGGL((adamw8_kernel<T, true, FAST>), grid, dim3(kNT), 0, s, p, g, cm, am, cv, av, master, n, hyper,
                       gsp, ioff);
  else
    hipLaunchKernelGGL((adamw8_kernel<T, false, FAST>), grid, dim3(kNT), 0, s, p, g, cm, am, cv, av, master, n, hyper,
                       gsp, ioff);
}

}  // namespace

void adamw8_step(DType dt, void* p, const void* g, uint8_t* codes_m, float* absmax_m, uint8_t* codes_v,
                 float* absmax_v, float* master, int64_t n, const float* hyper, const float* gsp, hipStream_t s,
                 int max_blocks, int64_t ioff) {
  const dim3 grid(q8_grid(n, kChunk, max_blocks));
  const uint64_t io = (uint64_t)ioff;
  const bool fast = adamw_fastmath();
  if (dt == DType::BF16) {
    if (fast)
      launch_adamw8<bf16, true>(grid, s, (bf16*)p, (const bf16*)g, codes_m, absmax_m, codes_v, absmax_v, master, n,
                                hyper, gsp, io);
    else
      launch_adamw8<bf16, false>(grid, s, (bf16*)p, (const bf16*)g, codes_m, absmax_m, codes_v, absmax_v, master, n,
                                 hyper, gsp, io);
  } else {
    if (fast)
      launch_adamw8<float, true>(grid, s, (float*)p, (const float*)g, codes_m, absmax_m, codes_v, absmax_v, master, n,
                                 hyper, gsp, io);
    else
      launch_adamw8<float, false>(grid, s, (float*)p, (const float*)g, codes_m, absmax_m, codes_v, absmax_v, master,
                                  n, hyper, gsp, io);
  }
}

void quantize_blockwise8(const float* x, uint8_t* codes, float* absmax, int64_t n, bool is_signed, hipStream_t s) {
  const dim3 grid(q8_grid(n, kChunk, 0));
  if (is_signed)
    hipLaunchKernelGGL(quantize8_kernel<true>, grid, dim3(kNT), 0, s, x, codes, absmax, n);
  else
    hipLaunchKernelGGL(quantize8_kernel<false>, grid, dim3(kNT), 0, s, x, codes, absmax, n);
}

void dequantize_blockwise8(const uint8_t* codes, const float* absmax, float* out, int64_t n, bool is_signed,
                           hipStream_t s) {
  const dim3 grid(q8_grid(n, kNT, 0));
  if (is_signed)
    hipLaunchKernelGGL(dequantize8_kernel<true>, grid, dim3(kNT), 0, s, codes, absmax, out, n);
  else
    hipLaunchKernelGGL(dequantize8_kernel<false>, grid, dim3(kNT), 0, s, codes, absmax, out, n);
}

}  // namespace grt
