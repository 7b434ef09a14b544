// torch <-> HIP kernel bindings for gke_ray_train_amd._C.
//
// Every op launches on the caller's current HIP stream (graph-capturable: no allocation
// besides the torch caching allocator, no synchronisation) and checks shapes/strides on the
// host BEFORE launch so a hand-written kernel never sees operands its grid does not expect.
#include <climits>
#include <torch/extension.h>

#include <algorithm>
#include <cmath>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include "grt_kernels.h"
#include "grt_sdma.h"

namespace {

using at::Tensor;
using c10::optional;

hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

grt::DType dtype_of(const Tensor& t) {
  if (t.scalar_type() == at::kBFloat16) return grt::DType::BF16;
  TORCH_CHECK(t.scalar_type() == at::kFloat, "gke_ray_train_amd kernels support bf16/fp32, got ", t.scalar_type());
  return grt::DType::F32;
}

void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
}
void check_contig(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_vec(const Tensor& t, int64_t d, const char* name) {
  const int64_t vec = t.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(d % vec == 0, name, ": last dim ", d, " must be a multiple of ", vec);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}
const void* ptr_or_null(const optional<Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

// ------------------------------------------------------------------ norms
// The norm kernels index every operand from the row tensor's shape alone, so each binding checks
// every operand against it first: rows [rows, d] (x / h; residual, dy, dres like it), per-feature
// vectors [d] (w, b) and per-row fp32 statistics [rows] (mean, rstd).

// the row tensor: bf16 / fp32, contiguous, 16-byte rows, no wider than the dispatch ladders of
// norm.hip cover (a wider row would lose its tail silently); returns d
int64_t check_norm_rows(const Tensor& t, const char* name) {
  check_contig(t, name);
  dtype_of(t);
  TORCH_CHECK(t.dim() >= 1 && t.size(-1) > 0, name, " must be [..., d] with d > 0");
  const int64_t d = t.size(-1);
  check_vec(t, d, name);
  const int64_t vec = t.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(d / vec <= grt::norm_max_chunks(), name, ": last dim ", d, " is wider than the norm kernels' limit of ",
              grt::norm_max_chunks(), " 16-byte chunks (", grt::norm_max_chunks() * vec, " elements of ",
              t.scalar_type(), ")");
  return d;
}
void check_norm_like(const Tensor& t, const Tensor& rows_t, const char* name) {
  check_contig(t, name);
  TORCH_CHECK(t.sizes() == rows_t.sizes() && t.scalar_type() == rows_t.scalar_type() && t.device() == rows_t.device(),
              name, " must match the input's shape, dtype and device");
}
void check_norm_param(const Tensor& t, const Tensor& rows_t, int64_t d, const char* name) {
  check_contig(t, name);
  TORCH_CHECK(t.numel() == d && t.scalar_type() == rows_t.scalar_type() && t.device() == rows_t.device(), name,
              " must hold ", d, " elements in the input's dtype on its device");
}
void check_norm_stat(const Tensor& t, const Tensor& rows_t, int64_t rows, const char* name) {
  check_contig(t, name);
  TORCH_CHECK(t.numel() == rows && t.scalar_type() == at::kFloat && t.device() == rows_t.device(), name,
              " must hold one fp32 value per row (", rows, ") on the input's device");
}

// pad > 0: y is the [rows, d] view of a [rows, d + pad] buffer (row stride d + pad) whose last pad
// columns a consumer fills (the LoRA h of a K-concatenated projection, peft/lora.py)
std::vector<Tensor> rmsnorm_fwd(const Tensor& x, const optional<Tensor>& residual, const Tensor& w,
                                double eps, int64_t pad) {
  const int64_t d = check_norm_rows(x, "x"), rows = x.numel() / d;
  check_norm_param(w, x, d, "w");
  c10::OptionalDeviceGuard g(x.device());
  TORCH_CHECK(pad >= 0 && pad % 8 == 0 && (pad == 0 || x.dim() == 2), "rmsnorm_fwd: pad % 8 == 0 on [rows, d]");
  auto y = pad == 0 ? at::empty_like(x) : at::empty({rows, d + pad}, x.options()).narrow(1, 0, d);
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  Tensor h;
  if (residual.has_value()) {
    check_norm_like(*residual, x, "residual");
    h = at::empty_like(x);
  }
  if (rows == 0) return {y, residual.has_value() ? h : x, rstd};
  grt::rmsnorm_fwd(dtype_of(x), x.data_ptr(), ptr_or_null(residual), w.data_ptr(), y.data_ptr(),
                   residual.has_value() ? h.data_ptr() : nullptr, rstd.data_ptr<float>(), rows, (int)d,
                   (float)eps, cur_stream(x), d + pad);
  return {y, residual.has_value() ? h : x, rstd};
}

// dw_out given: the weight gradient goes straight into it (parameter dtype, e.g. a data-parallel
// gradient slot; accumulate adds) and the second result is dw_out itself.
std::vector<Tensor> rmsnorm_bwd(const Tensor& dy, const Tensor& h, const Tensor& w, const Tensor& rstd,
                                const optional<Tensor>& dres, const optional<Tensor>& dw_out, bool accumulate) {
  const int64_t d = check_norm_rows(h, "h"), rows = h.numel() / d;
  check_norm_like(dy, h, "dy");
  check_norm_param(w, h, d, "w");
  check_norm_stat(rstd, h, rows, "rstd");
  if (dres.has_value()) check_norm_like(*dres, h, "dres");
  if (dw_out.has_value()) check_norm_param(*dw_out, h, d, "dw_out");
  c10::OptionalDeviceGuard g(h.device());
  auto dx = at::empty_like(h);
  if (rows == 0) {  // nothing to sum: a zero gradient, or dw_out as it is when accumulating
    if (!dw_out.has_value()) return {dx, at::zeros({d}, h.options().dtype(at::kFloat))};
    if (!accumulate) dw_out->zero_();
    return {dx, *dw_out};
  }
  Tensor dw = dw_out.has_value() ? *dw_out : at::empty({d}, h.options().dtype(at::kFloat));
  auto ws = at::empty({grt::norm_bwd_workspace_floats(rows, (int)d)}, h.options().dtype(at::kFloat));
  grt::rmsnorm_bwd(dtype_of(h), dy.data_ptr(), h.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(),
                   ptr_or_null(dres), dx.data_ptr(), dw_out.has_value() ? nullptr : dw.data_ptr<float>(),
                   ws.data_ptr<float>(), rows, (int)d, cur_stream(h),
                   dw_out.has_value() ? dw.data_ptr() : nullptr, accumulate ? 1 : 0);
  return {dx, dw};
}

// dX only (frozen norm weight: LoRA / QLoRA): no weight-gradient slab, no column-sum launch
Tensor rmsnorm_bwd_dx(const Tensor& dy, const Tensor& h, const Tensor& w, const Tensor& rstd,
                      const optional<Tensor>& dres) {
  const int64_t d = check_norm_rows(h, "h"), rows = h.numel() / d;
  check_norm_like(dy, h, "dy");
  check_norm_param(w, h, d, "w");
  check_norm_stat(rstd, h, rows, "rstd");
  if (dres.has_value()) check_norm_like(*dres, h, "dres");
  c10::OptionalDeviceGuard g(h.device());
  auto dx = at::empty_like(h);
  if (rows == 0) return dx;
  grt::rmsnorm_bwd(dtype_of(h), dy.data_ptr(), h.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(),
                   ptr_or_null(dres), dx.data_ptr(), nullptr, nullptr, rows, (int)d, cur_stream(h), nullptr, 0);
  return dx;
}

std::vector<Tensor> layernorm_fwd(const Tensor& x, const optional<Tensor>& residual, const Tensor& w,
                                  const optional<Tensor>& b, double eps) {
  const int64_t d = check_norm_rows(x, "x"), rows = x.numel() / d;
  check_norm_param(w, x, d, "w");
  if (b.has_value()) check_norm_param(*b, x, d, "b");
  c10::OptionalDeviceGuard g(x.device());
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  Tensor h;
  if (residual.has_value()) {
    check_norm_like(*residual, x, "residual");
    h = at::empty_like(x);
  }
  if (rows == 0) return {y, residual.has_value() ? h : x, mean, rstd};
  grt::layernorm_fwd(dtype_of(x), x.data_ptr(), ptr_or_null(residual), w.data_ptr(), ptr_or_null(b),
                     y.data_ptr(), residual.has_value() ? h.data_ptr() : nullptr, mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), rows, (int)d, (float)eps, cur_stream(x));
  return {y, residual.has_value() ? h : x, mean, rstd};
}

std::vector<Tensor> layernorm_bwd(const Tensor& dy, const Tensor& h, const Tensor& w, const Tensor& mean,
                                  const Tensor& rstd, const optional<Tensor>& dres) {
  const int64_t d = check_norm_rows(h, "h"), rows = h.numel() / d;
  check_norm_like(dy, h, "dy");
  check_norm_param(w, h, d, "w");
  check_norm_stat(mean, h, rows, "mean");
  check_norm_stat(rstd, h, rows, "rstd");
  if (dres.has_value()) check_norm_like(*dres, h, "dres");
  c10::OptionalDeviceGuard g(h.device());
  auto dx = at::empty_like(h);
  if (rows == 0) {
    auto z = at::zeros({d}, h.options().dtype(at::kFloat));
    return {dx, z, at::zeros_like(z)};
  }
  auto dw = at::empty({d}, h.options().dtype(at::kFloat));
  auto db = at::empty({d}, h.options().dtype(at::kFloat));
  auto ws = at::empty({grt::norm_bwd_workspace_floats(rows, (int)d)}, h.options().dtype(at::kFloat));
  grt::layernorm_bwd(dtype_of(h), dy.data_ptr(), h.data_ptr(), w.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), ptr_or_null(dres), dx.data_ptr(), dw.data_ptr<float>(),
                     db.data_ptr<float>(), ws.data_ptr<float>(), rows, (int)d, cur_stream(h));
  return {dx, dw, db};
}

// ------------------------------------------------------------------ elementwise
Tensor swiglu_fwd(const Tensor& gu, int64_t pad) {  // pad: as rmsnorm_fwd (a LoRA-tail row buffer)
  check_contig(gu, "gu");
  c10::OptionalDeviceGuard g(gu.device());
  const int64_t two_f = gu.size(-1), rows = gu.numel() / two_f, f = two_f / 2;
  check_vec(gu, f, "gu");
  TORCH_CHECK(pad >= 0 && pad % 8 == 0 && (pad == 0 || gu.dim() == 2), "swiglu_fwd: pad % 8 == 0 on [rows, 2f]");
  auto sizes = gu.sizes().vec();
  sizes.back() = f;
  auto out = pad == 0 ? at::empty(sizes, gu.options()) : at::empty({rows, f + pad}, gu.options()).narrow(1, 0, f);
  grt::swiglu_fwd(dtype_of(gu), gu.data_ptr(), out.data_ptr(), rows, (int)f, cur_stream(gu), f + pad);
  return out;
}
Tensor swiglu_bwd(const Tensor& gu, const Tensor& dout) {
  check_contig(gu, "gu");
  check_contig(dout, "dout");
  c10::OptionalDeviceGuard g(gu.device());
  const int64_t two_f = gu.size(-1), rows = gu.numel() / two_f, f = two_f / 2;
  check_vec(gu, f, "gu");
  TORCH_CHECK(dout.numel() == rows * f && dout.scalar_type() == gu.scalar_type() && dout.device() == gu.device(),
              "dout shape / dtype / device mismatch");
  check_vec(dout, f, "dout");
  auto dgu = at::empty_like(gu);
  grt::swiglu_bwd(dtype_of(gu), gu.data_ptr(), dout.data_ptr(), dgu.data_ptr(), rows, (int)f, cur_stream(gu));
  return dgu;
}
// (out, out^T) or None when the shape is not handled
std::vector<Tensor> swiglu_fwd_t(const Tensor& gu, int64_t pad) {
  check_contig(gu, "gu");
  c10::OptionalDeviceGuard g(gu.device());
  const int64_t two_f = gu.size(-1), rows = gu.numel() / two_f, f = two_f / 2;
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 && gu.is_cuda(), "swiglu_fwd_t: bf16 on the device");
  TORCH_CHECK(pad >= 0 && pad % 8 == 0 && (pad == 0 || gu.dim() == 2), "swiglu_fwd_t: pad % 8 == 0 on [rows, 2f]");
  if (rows % 64 != 0 || f % 128 != 0 || reinterpret_cast<uintptr_t>(gu.data_ptr()) % 16 != 0) return {};
  auto sizes = gu.sizes().vec();
  sizes.back() = f;
  auto out = pad == 0 ? at::empty(sizes, gu.options()) : at::empty({rows, f + pad}, gu.options()).narrow(1, 0, f);
  auto outT = at::empty({f, rows}, gu.options());
  if (!grt::swiglu_fwd_t(gu.data_ptr(), out.data_ptr(), outT.data_ptr(), rows, (int)f, cur_stream(gu), f + pad))
    return {};
  return {out, outT};
}
// (dgu, dgu^T) or None when the shape is not handled
std::vector<Tensor> swiglu_bwd_t(const Tensor& gu, const Tensor& dout) {
  check_contig(gu, "gu");
  check_contig(dout, "dout");
  c10::OptionalDeviceGuard g(gu.device());
  const int64_t two_f = gu.size(-1), rows = gu.numel() / two_f, f = two_f / 2;
  TORCH_CHECK(dout.numel() == rows * f && dout.scalar_type() == gu.scalar_type(), "dout shape mismatch");
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 && gu.is_cuda(), "swiglu_bwd_t: bf16 on the device");
  if (rows % 64 != 0 || f % 128 != 0 || reinterpret_cast<uintptr_t>(gu.data_ptr()) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 != 0)
    return {};
  auto dgu = at::empty_like(gu);
  auto dguT = at::empty({two_f, rows}, gu.options());
  if (!grt::swiglu_bwd_t(gu.data_ptr(), dout.data_ptr(), dgu.data_ptr(), dguT.data_ptr(), rows, (int)f, cur_stream(gu)))
    return {};
  return {dgu, dguT};
}
Tensor gelu_fwd(const Tensor& x) {
  check_contig(x, "x");
  c10::OptionalDeviceGuard g(x.device());
  check_vec(x, x.numel(), "x");
  auto y = at::empty_like(x);
  grt::gelu_fwd(dtype_of(x), x.data_ptr(), y.data_ptr(), x.numel(), cur_stream(x));
  return y;
}
Tensor gelu_bwd(const Tensor& x, const Tensor& dy) {
  check_contig(x, "x");
  check_contig(dy, "dy");
  c10::OptionalDeviceGuard g(x.device());
  check_vec(x, x.numel(), "x");
  auto dx = at::empty_like(x);
  grt::gelu_bwd(dtype_of(x), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), cur_stream(x));
  return dx;
}

void check_rope(const Tensor& cos, const Tensor& sin, const optional<Tensor>& pos, int64_t T, int64_t S, int64_t D) {
  check_contig(cos, "cos");
  check_contig(sin, "sin");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat, "cos/sin must be fp32");
  TORCH_CHECK(cos.size(-1) == D / 2 && cos.numel() >= S * (D / 2) && sin.sizes() == cos.sizes(), "cos/sin shape");
  TORCH_CHECK(D % 16 == 0, "head_dim must be a multiple of 16");
  if (pos.has_value()) {
    check_contig(*pos, "pos");
    TORCH_CHECK(pos->scalar_type() == at::kInt && pos->numel() == T, "pos must be int32 [T]");
  }
}

// qkv: [T, ld] (row-contiguous), returns q [T, hq, D], k [T, hkv, D]
std::vector<Tensor> rope_fwd(const Tensor& qkv, const Tensor& cos, const Tensor& sin,
                             const optional<Tensor>& pos, int64_t hq, int64_t hkv, int64_t D, int64_t S) {
  check_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1, "qkv must be [T, ld] with unit column stride");
  c10::OptionalDeviceGuard g(qkv.device());
  const int64_t T = qkv.size(0), ld = qkv.stride(0);
  TORCH_CHECK(qkv.size(1) >= (hq + hkv) * D, "qkv too narrow");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "qkv alignment");
  check_rope(cos, sin, pos, T, S, D);
  auto q = at::empty({T, hq, D}, qkv.options());
  auto k = at::empty({T, hkv, D}, qkv.options());
  if (T == 0) return {q, k};
  grt::rope_fwd(dtype_of(qkv), qkv.data_ptr(), ld, q.data_ptr(), k.data_ptr(), cos.data_ptr<float>(),
                sin.data_ptr<float>(), pos.has_value() ? pos->data_ptr<int32_t>() : nullptr, T, (int)S,
                (int)hq, (int)hkv, (int)D, cur_stream(qkv));
  return {q, k};
}

// decode: q = rope(q) [T, hq, D]; kc[t / tpr, pos[t]] = rope(k), vc[t / tpr, pos[t]] = v (caches
// [B, L, hkv, D], last dim contiguous); a token whose position is outside [0, min(S, L)) is skipped
// entirely by the kernel (no cache write, its q row left unwritten)
Tensor rope_append(const Tensor& qkv, const Tensor& cos, const Tensor& sin, const Tensor& pos, int64_t hq, int64_t hkv,
                   int64_t D, int64_t S, Tensor& kc, Tensor& vc, int64_t tpr) {
  check_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1 && qkv.scalar_type() == at::kBFloat16, "qkv must be bf16 [T, ld]");
  c10::OptionalDeviceGuard g(qkv.device());
  const int64_t T = qkv.size(0), ld = qkv.stride(0);
  TORCH_CHECK(qkv.size(1) >= (hq + 2 * hkv) * D && D % 16 == 0, "qkv too narrow / head dim");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "qkv alignment");
  check_rope(cos, sin, pos, T, S, D);
  for (const Tensor* c : {&kc, &vc}) {
    check_cuda(*c, "cache");
    TORCH_CHECK(c->dim() == 4 && c->size(2) == hkv && c->size(3) == D && c->stride(3) == 1 &&
                c->scalar_type() == at::kBFloat16, "cache must be bf16 [B, L, hkv, D] with unit last stride");
    TORCH_CHECK(c->stride(0) % 8 == 0 && c->stride(1) % 8 == 0 && c->stride(2) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, "cache alignment");
  }
  TORCH_CHECK(tpr >= 1 && T % tpr == 0 && T / tpr == kc.size(0) && vc.sizes() == kc.sizes(),
              "rope_append: T = B * tokens-per-row");
  auto q = at::empty({T, hq, D}, qkv.options());
  grt::rope_append(qkv.data_ptr(), ld, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kc.stride(1),
                   kc.stride(2), vc.stride(0), vc.stride(1), vc.stride(2), cos.data_ptr<float>(), sin.data_ptr<float>(),
                   pos.data_ptr<int32_t>(), T, (int)tpr, (int)S, (int)kc.size(1), (int)hq, (int)hkv, (int)D,
                   cur_stream(qkv));
  return q;
}

// fp8 KV cache (kv_fp8.hip): codes uint8 [B, L, hkv, D] with unit last stride and 8-byte aligned
// base and strides, scales fp32 [B, L, hkv] on the same device
void check_fp8_cache(const Tensor& c, const Tensor& sc, const Tensor& like, const char* op, const char* name) {
  check_cuda(c, name);
  check_cuda(sc, name);
  TORCH_CHECK(c.scalar_type() == at::kByte && c.dim() == 4 && c.stride(3) == 1, op, ": ", name,
              " must be uint8 codes [B, L, Hkv, D] with unit last stride");
  TORCH_CHECK(sc.scalar_type() == at::kFloat && sc.dim() == 3 && sc.size(0) == c.size(0) && sc.size(1) == c.size(1) &&
                  sc.size(2) == c.size(2),
              op, ": ", name, " scales must be fp32 [B, L, Hkv]");
  TORCH_CHECK(c.device() == like.device() && sc.device() == like.device(), op, ": ", name, " on the same device");
  TORCH_CHECK(c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 && c.stride(2) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(c.data_ptr()) % 8 == 0,
              op, ": ", name, " needs an 8-byte aligned base pointer and strides");
}

// rope_append into an fp8 cache: K is rotated, rounded to bf16 and quantised, V quantised; k_out
// (optional, bf16 [T, hkv, D] contiguous) receives the rotated bf16 K (the prefill attends over it)
Tensor rope_append_fp8(const Tensor& qkv, const Tensor& cos, const Tensor& sin, const Tensor& pos, int64_t hq,
                       int64_t hkv, int64_t D, int64_t S, Tensor& kc, Tensor& vc, Tensor& k_scale, Tensor& v_scale,
                       int64_t tpr, const optional<Tensor>& k_out) {
  const char* op = "rope_append_fp8";
  check_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1 && qkv.scalar_type() == at::kBFloat16, "qkv must be bf16 [T, ld]");
  c10::OptionalDeviceGuard g(qkv.device());
  const int64_t T = qkv.size(0), ld = qkv.stride(0);
  TORCH_CHECK(qkv.size(1) >= (hq + 2 * hkv) * D && (D == 64 || D == 128), op, ": qkv too narrow / head_dim 64 or 128");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "qkv alignment");
  check_rope(cos, sin, pos, T, S, D);
  check_fp8_cache(kc, k_scale, qkv, op, "k cache");
  check_fp8_cache(vc, v_scale, qkv, op, "v cache");
  TORCH_CHECK(kc.size(2) == hkv && kc.size(3) == D && vc.sizes() == kc.sizes(), op, ": caches must be [B, L, hkv, D]");
  TORCH_CHECK(tpr >= 1 && T % tpr == 0 && T / tpr == kc.size(0), op, ": T = B * tokens-per-row");
  TORCH_CHECK(kc.size(1) <= INT32_MAX && hq >= 0 && hkv >= 1, op, ": dims");
  auto q = at::empty({T, hq, D}, qkv.options());
  grt::RopeAppendFp8Params a{};
  a.qkv = qkv.data_ptr(); a.ld = ld; a.q_out = q.data_ptr(); a.k_out = nullptr;
  if (k_out.has_value()) {
    check_contig(*k_out, "k_out");
    TORCH_CHECK(k_out->scalar_type() == at::kBFloat16 && k_out->numel() == T * hkv * D && k_out->device() == qkv.device() &&
                    reinterpret_cast<uintptr_t>(k_out->data_ptr()) % 16 == 0,
                op, ": k_out must be a contiguous bf16 [T, hkv, D]");
    a.k_out = k_out->data_ptr();
  }
  a.kc = kc.data_ptr(); a.vc = vc.data_ptr(); a.k_scale = k_scale.data_ptr<float>(); a.v_scale = v_scale.data_ptr<float>();
  a.c_bs = kc.stride(0); a.c_ss = kc.stride(1); a.c_hs = kc.stride(2);
  a.v_bs = vc.stride(0); a.v_ss = vc.stride(1); a.v_hs = vc.stride(2);
  a.ks_bs = k_scale.stride(0); a.ks_ss = k_scale.stride(1); a.ks_hs = k_scale.stride(2);
  a.vs_bs = v_scale.stride(0); a.vs_ss = v_scale.stride(1); a.vs_hs = v_scale.stride(2);
  a.cos = cos.data_ptr<float>(); a.sin = sin.data_ptr<float>(); a.pos = pos.data_ptr<int32_t>();
  a.T = T; a.tpr = (int)tpr; a.S = (int)S; a.L = (int)kc.size(1); a.hq = (int)hq; a.hkv = (int)hkv; a.D = (int)D;
  grt::rope_append_fp8(a, cur_stream(qkv));
  return q;
}

// rows [0, n) of an fp8 cache as bf16 [B, n, Hkv, D]
Tensor kv_fp8_dequant(const Tensor& codes, const Tensor& scale, int64_t n) {
  check_fp8_cache(codes, scale, codes, "kv_fp8_dequant", "cache");
  TORCH_CHECK(n >= 0 && n <= codes.size(1) && codes.size(3) % 8 == 0 && codes.size(1) <= INT32_MAX, "kv_fp8_dequant: n / head_dim");
  c10::OptionalDeviceGuard g(codes.device());
  auto out = at::empty({codes.size(0), n, codes.size(2), codes.size(3)}, codes.options().dtype(at::kBFloat16));
  grt::kv_fp8_dequant(codes.data_ptr(), scale.data_ptr<float>(), out.data_ptr(), codes.stride(0), codes.stride(1),
                      codes.stride(2), scale.stride(0), scale.stride(1), scale.stride(2), codes.size(0), (int)n,
                      (int)codes.size(2), (int)codes.size(3), cur_stream(codes));
  return out;
}

void rope_bwd(const Tensor& dq, const Tensor& dk, Tensor& dqkv, const Tensor& cos, const Tensor& sin,
              const optional<Tensor>& pos, int64_t hq, int64_t hkv, int64_t D, int64_t S) {
  check_contig(dq, "dq");
  check_contig(dk, "dk");
  check_cuda(dqkv, "dqkv");
  TORCH_CHECK(dqkv.dim() == 2 && dqkv.stride(1) == 1, "dqkv must be [T, ld] with unit column stride");
  TORCH_CHECK(dk.scalar_type() == dq.scalar_type() && dqkv.scalar_type() == dq.scalar_type() &&
              dk.device() == dq.device() && dqkv.device() == dq.device(), "dq / dk / dqkv must share dtype and device");
  c10::OptionalDeviceGuard g(dq.device());
  const int64_t T = dqkv.size(0), ld = dqkv.stride(0);
  TORCH_CHECK(dq.numel() == T * hq * D && dk.numel() == T * hkv * D, "dq/dk shape");
  TORCH_CHECK(dqkv.size(1) >= (hq + hkv) * D, "dqkv too narrow");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(dqkv.data_ptr()) % 16 == 0, "dqkv alignment");
  check_rope(cos, sin, pos, T, S, D);
  if (T == 0) return;
  grt::rope_bwd(dtype_of(dq), dq.data_ptr(), dk.data_ptr(), dqkv.data_ptr(), ld, cos.data_ptr<float>(),
                sin.data_ptr<float>(), pos.has_value() ? pos->data_ptr<int32_t>() : nullptr, T, (int)S,
                (int)hq, (int)hkv, (int)D, cur_stream(dq));
}

Tensor scale_add_pe(const Tensor& emb, const optional<Tensor>& pe, int64_t S, double scale) {
  check_contig(emb, "emb");
  c10::OptionalDeviceGuard g(emb.device());
  const int64_t d = emb.size(-1), T = emb.numel() / d;
  check_vec(emb, d, "emb");
  if (pe.has_value()) {
    check_contig(*pe, "pe");
    TORCH_CHECK(pe->scalar_type() == at::kFloat && pe->numel() >= S * d, "pe must be fp32 [>=S, d]");
  }
  auto out = at::empty_like(emb);
  grt::scale_add_pe(dtype_of(emb), emb.data_ptr(), pe.has_value() ? pe->data_ptr<float>() : nullptr,
                    out.data_ptr(), T, (int)S, (int)d, (float)scale, cur_stream(emb));
  return out;
}

void check_drop_p(double p) { TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1), got ", p); }

std::vector<Tensor> dropout_fwd(const Tensor& x, double p, int64_t seed, int64_t offset) {
  check_contig(x, "x");
  check_drop_p(p);
  c10::OptionalDeviceGuard g(x.device());
  auto y = at::empty_like(x);
  auto mask = at::empty(x.sizes(), x.options().dtype(at::kByte));
  grt::dropout_fwd(dtype_of(x), x.data_ptr(), y.data_ptr(), mask.data_ptr<uint8_t>(), x.numel(), (float)p,
                   (uint64_t)seed, (uint64_t)offset, cur_stream(x));
  return {y, mask};
}
Tensor dropout_bwd(const Tensor& dy, const Tensor& mask, double p) {
  check_contig(dy, "dy");
  check_drop_p(p);
  TORCH_CHECK(mask.numel() == dy.numel(), "dropout_bwd: mask / dy sizes differ");
  check_contig(mask, "mask");
  c10::OptionalDeviceGuard g(dy.device());
  auto dx = at::empty_like(dy);
  grt::dropout_bwd(dtype_of(dy), dy.data_ptr(), mask.data_ptr<uint8_t>(), dx.data_ptr(), dy.numel(), (float)p,
                   cur_stream(dy));
  return dx;
}
// mask-free variants: forward stores no mask; backward regenerates it and can accumulate into dx
Tensor dropout_fwd_seeded(const Tensor& x, double p, int64_t seed, int64_t offset) {
  check_contig(x, "x");
  check_drop_p(p);
  c10::OptionalDeviceGuard g(x.device());
  auto y = at::empty_like(x);
  grt::dropout_fwd(dtype_of(x), x.data_ptr(), y.data_ptr(), nullptr, x.numel(), (float)p, (uint64_t)seed,
                   (uint64_t)offset, cur_stream(x));
  return y;
}
void dropout_bwd_seeded(const Tensor& dy, const Tensor& dx, double p, int64_t seed, int64_t offset, bool accumulate) {
  check_contig(dy, "dy");
  check_contig(dx, "dx");
  check_drop_p(p);
  TORCH_CHECK(dy.numel() == dx.numel() && dy.scalar_type() == dx.scalar_type(), "dropout_bwd_seeded: shapes");
  c10::OptionalDeviceGuard g(dy.device());
  grt::dropout_bwd(dtype_of(dy), dy.data_ptr(), nullptr, dx.data_ptr(), dy.numel(), (float)p, cur_stream(dy),
                   (uint64_t)seed, (uint64_t)offset, accumulate);
}

// ------------------------------------------------------------------ LoRA adapter
// compute units of a device (cached)
static int device_cus(int dev) {
  static int cache[64] = {0};
  if (dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cache[dev] = v;
  }
  return cache[dev];
}

// (h, xd) = lora_down(x [M, K], a [R, K]): h = (x * keep / (1-p)) a^T, xd = x * keep / (1-p) when
// want_xd (same keep mask as dropout_fwd_seeded(x, p, seed, offset)). Returns {} when the shape is
// not supported by the kernel (the caller falls back to the torch path).
std::vector<Tensor> lora_down(const Tensor& x, const Tensor& a, double p, int64_t seed, int64_t offset,
                              bool want_xd, const optional<Tensor>& h_out, double hscale) {
  check_cuda(x, "x");
  check_contig(a, "a");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1 && a.dim() == 2 && a.size(1) == x.size(1), "lora_down: shapes");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && a.scalar_type() == at::kBFloat16, "lora_down: bf16");
  check_drop_p(p);
  const int64_t M = x.size(0);
  const int K = (int)x.size(1), R = (int)a.size(0);
  if (!grt::lora_down_supported(M, K, R, (int)x.stride(0), (uint64_t)offset) ||
      reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 || reinterpret_cast<uintptr_t>(a.data_ptr()) % 16)
    return {};
  c10::OptionalDeviceGuard g(x.device());
  Tensor h;
  if (h_out.has_value()) {  // e.g. the LoRA tail of the [x | h] row buffer (row stride > R)
    h = *h_out;
    TORCH_CHECK(h.dim() == 2 && h.size(0) == M && h.size(1) == R && h.stride(1) == 1 && h.stride(0) % 8 == 0 &&
                    h.scalar_type() == at::kBFloat16 && reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0,
                "lora_down: h_out must be bf16 [M, R], unit column stride, 16-byte aligned rows");
  } else {
    h = at::empty({M, R}, x.options());
  }
  Tensor xd;
  if (want_xd) xd = at::empty({M, K}, x.options());
  grt::LoraDownParams lp{};
  lp.x = x.data_ptr(); lp.a = a.data_ptr(); lp.h = h.data_ptr(); lp.xd = want_xd ? xd.data_ptr() : nullptr;
  lp.M = M; lp.K = K; lp.R = R; lp.ldx = (int)x.stride(0);
  lp.p = (float)p; lp.seed = (uint64_t)seed; lp.offset = (uint64_t)offset;
  lp.ldh = h.stride(0); lp.hscale = (float)hscale;
  lp.ksplit = grt::lora_down_splits(M, K, R, device_cus(x.device().index()));
  Tensor hpart;
  if (lp.ksplit > 1) {
    hpart = at::empty({(int64_t)lp.ksplit, M, R}, x.options().dtype(at::kFloat));
    lp.hpart = hpart.data_ptr<float>();
  }
  grt::lora_down(lp, cur_stream(x));
  if (want_xd) return {h, xd};
  return {h};
}

// dx [M, K] (+)= keep / (1-p) * (g [M, R] @ at^T), at = A^T [K, R]; returns false (nothing done)
// when the shape is not supported by the kernel.
// g and dx may be row-strided (unit column stride); dx_in given: dx = dx_in + ... (dx_in row-strided too)
bool lora_dx(const Tensor& g, const Tensor& at, const Tensor& dx, double p, int64_t seed, int64_t offset,
             bool accumulate, const optional<Tensor>& dx_in, double gscale) {
  check_contig(at, "at");
  for (const Tensor* t : {&g, &dx}) {
    check_cuda(*t, "lora_dx operand");
    TORCH_CHECK(t->dim() == 2 && t->stride(1) == 1 && t->stride(0) % 8 == 0, "lora_dx: row-major operands");
  }
  if (dx_in.has_value()) {
    TORCH_CHECK(dx_in->sizes() == dx.sizes() && dx_in->stride(1) == 1 && dx_in->stride(0) % 8 == 0 &&
                    dx_in->scalar_type() == at::kBFloat16 && reinterpret_cast<uintptr_t>(dx_in->data_ptr()) % 16 == 0,
                "lora_dx: dx_in like dx");
  }
  TORCH_CHECK(g.dim() == 2 && at.dim() == 2 && dx.dim() == 2 && g.size(0) == dx.size(0) &&
                  at.size(0) == dx.size(1) && at.size(1) == g.size(1), "lora_dx: shapes");
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 && at.scalar_type() == at::kBFloat16 &&
                  dx.scalar_type() == at::kBFloat16, "lora_dx: bf16");
  check_drop_p(p);
  const int64_t M = dx.size(0);
  const int K = (int)dx.size(1), R = (int)g.size(1);
  if (!grt::lora_dx_supported(M, K, R, (uint64_t)offset) || reinterpret_cast<uintptr_t>(dx.data_ptr()) % 16 ||
      reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 || reinterpret_cast<uintptr_t>(at.data_ptr()) % 16)
    return false;
  c10::OptionalDeviceGuard dg(dx.device());
  grt::LoraDxParams lp{};
  lp.g = g.data_ptr(); lp.at = at.data_ptr(); lp.dx = dx.data_ptr();
  lp.M = M; lp.K = K; lp.R = R;
  lp.p = (float)p; lp.seed = (uint64_t)seed; lp.offset = (uint64_t)offset; lp.accumulate = accumulate ? 1 : 0;
  lp.ldg = g.stride(0); lp.ld_out = dx.stride(0); lp.gscale = (float)gscale;
  if (dx_in.has_value()) { lp.dx_in = dx_in->data_ptr(); lp.ld_in = dx_in->stride(0); }
  grt::lora_dx(lp, cur_stream(dx));
  return true;
}

static bool rowmajor_bf16(const Tensor& t) {
  return t.is_cuda() && t.dim() == 2 && t.scalar_type() == at::kBFloat16 && t.stride(1) == 1 &&
         t.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// c [M, 64] (+)= alpha * a [M, K] @ bt^T, bt = B^T [64, K] (lora_grad.hip); all row-major with unit
// column stride (row-strided views allowed). Returns false (nothing done) when unsupported.
// lora_g_group: up to 4 such products of the same M (one adapted module's targets) in one launch.
static bool lora_g_impl(const std::vector<Tensor>& as, const std::vector<Tensor>& bts, const std::vector<Tensor>& cs,
                        double alpha, bool accumulate) {
  const int n = (int)as.size();
  if (n < 1 || n > grt::kLoraGMax || (int)bts.size() != n || (int)cs.size() != n) return false;
  grt::LoraGParams p{};
  const int64_t M = as[0].size(0);
  int kmax = 0;
  for (int t = 0; t < n; ++t) {
    const Tensor &a = as[t], &bt = bts[t], &c = cs[t];
    if (!rowmajor_bf16(a) || !rowmajor_bf16(bt) || !rowmajor_bf16(c)) return false;
    const int K = (int)a.size(1);
    if (a.size(0) != M || bt.size(0) != c.size(1) || bt.size(1) != K || c.size(0) != M ||
        !grt::lora_g_supported(M, K, (int)c.size(1)) || c.stride(0) % 4 != 0 || c.get_device() != cs[0].get_device())
      return false;
    p.a[t] = a.data_ptr(); p.lda[t] = a.stride(0); p.bt[t] = bt.data_ptr(); p.ldbt[t] = bt.stride(0);
    p.c[t] = c.data_ptr(); p.ldc[t] = c.stride(0); p.K[t] = K;
    kmax = std::max(kmax, K);
  }
  for (int t = n; t < grt::kLoraGMax; ++t) {  // unused slots mirror product 0 (never indexed)
    p.a[t] = p.a[0]; p.lda[t] = p.lda[0]; p.bt[t] = p.bt[0]; p.ldbt[t] = p.ldbt[0];
    p.c[t] = p.c[0]; p.ldc[t] = p.ldc[0]; p.K[t] = p.K[0];
  }
  const Tensor& c0 = cs[0];
  c10::OptionalDeviceGuard dg(c0.device());
  p.nprod = n; p.M = M; p.alpha = (float)alpha; p.accumulate = accumulate ? 1 : 0;
  int kmin = kmax;
  for (int t = 0; t < n; ++t) kmin = std::min(kmin, p.K[t]);
  p.ks = grt::lora_g_splits(M, kmin, device_cus(c0.get_device()), n);
  Tensor ws;
  if (p.ks > 1) {
    ws = at::empty({(int64_t)n * p.ks * M * 64}, c0.options().dtype(at::kFloat));
    p.ws = ws.data_ptr<float>();
  }
  grt::lora_g(p, cur_stream(c0));
  return true;
}

bool lora_g(const Tensor& a, const Tensor& bt, const Tensor& c, double alpha, bool accumulate) {
  return lora_g_impl({a}, {bt}, {c}, alpha, accumulate);
}

bool lora_g_group(const std::vector<Tensor>& as, const std::vector<Tensor>& bts, const std::vector<Tensor>& cs,
                  double alpha, bool accumulate) {
  return lora_g_impl(as, bts, cs, alpha, accumulate);
}

// out (+)= alpha * a^T @ h, a [M, N], h [M, R]: out [N, R], or [R, N] when transpose (lora_grad.hip);
// fp32 token-split partials in a workspace from the caching allocator. False when unsupported.
// lora_tred_group: up to 4 such products of the same M and R (non-transposed; one adapted module's
// dB_i) in one launch, each assigning or accumulating.
static bool lora_tred_impl(const std::vector<Tensor>& as, const std::vector<Tensor>& hs, const std::vector<Tensor>& outs,
                           double alpha, const std::vector<bool>& accumulate, bool transpose) {
  const int n = (int)as.size();
  if (n < 1 || n > grt::kLoraTredMax || (int)hs.size() != n || (int)outs.size() != n || (int)accumulate.size() != n ||
      (transpose && n != 1))
    return false;
  const int64_t M = as[0].size(0);
  const int R = (int)hs[0].size(1);
  grt::LoraTredParams p{};
  int nbt = 0;
  for (int t = 0; t < n; ++t) {
    const Tensor &a = as[t], &h = hs[t], &out = outs[t];
    if (!rowmajor_bf16(a) || !rowmajor_bf16(h) || !rowmajor_bf16(out)) return false;
    const int N = (int)a.size(1);
    if (a.size(0) != M || h.size(0) != M || h.size(1) != R || !grt::lora_tred_supported(M, N, R)) return false;
    if (transpose ? (out.size(0) != R || out.size(1) != N) : (out.size(0) != N || out.size(1) != R)) return false;
    if (out.stride(0) % 4 != 0 || out.get_device() != outs[0].get_device()) return false;
    p.a[t] = a.data_ptr(); p.lda[t] = a.stride(0); p.h[t] = h.data_ptr(); p.ldh[t] = h.stride(0);
    p.out[t] = out.data_ptr(); p.ldo[t] = out.stride(0); p.N[t] = N; p.bo[t] = nbt;
    p.accumulate[t] = accumulate[t] ? 1 : 0;
    nbt += N / 128;
  }
  for (int t = n; t < grt::kLoraTredMax; ++t) {  // unused slots: never selected (bo past every block)
    p.a[t] = p.a[0]; p.lda[t] = p.lda[0]; p.h[t] = p.h[0]; p.ldh[t] = p.ldh[0];
    p.out[t] = p.out[0]; p.ldo[t] = p.ldo[0]; p.N[t] = p.N[0]; p.bo[t] = INT_MAX; p.accumulate[t] = 0;
  }
  const Tensor& o0 = outs[0];
  c10::OptionalDeviceGuard dg(o0.device());
  p.nprod = n; p.nbt = nbt; p.M = M; p.R = R;
  p.ks = grt::lora_tred_splits(M, nbt * 128, R, device_cus(o0.get_device()));
  Tensor ws = at::empty({(int64_t)p.ks * nbt * 128 * R}, o0.options().dtype(at::kFloat));
  p.ws = ws.data_ptr<float>();
  p.transpose = transpose ? 1 : 0; p.alpha = (float)alpha;
  grt::lora_tred(p, cur_stream(o0));
  return true;
}

bool lora_tred(const Tensor& a, const Tensor& h, const Tensor& out, double alpha, bool accumulate, bool transpose) {
  return lora_tred_impl({a}, {h}, {out}, alpha, {accumulate}, transpose);
}

bool lora_tred_group(const std::vector<Tensor>& as, const std::vector<Tensor>& hs, const std::vector<Tensor>& outs,
                     double alpha, const std::vector<bool>& accumulate) {
  return lora_tred_impl(as, hs, outs, alpha, accumulate, false);
}

// B_i [n_i, r] -> the adapter tail of W' [out, ldw] (columns col0 + j r ..) and of W'^T [.., ldt]
void lora_refresh(const std::vector<Tensor>& bs, const std::vector<int64_t>& offs, Tensor& w,
                  const optional<Tensor>& wt_opt, int64_t col0, int64_t wt_row0) {
  if (wt_row0 < 0) wt_row0 = col0;  // W'^T rows of the adapter block (a separate B^T buffer: 0)
  TORCH_CHECK(!bs.empty() && bs.size() <= 4 && offs.size() == bs.size(), "lora_refresh: 1-4 targets");
  TORCH_CHECK(w.dim() == 2 && w.stride(1) == 1 && w.scalar_type() == at::kBFloat16, "lora_refresh: bf16 W'");
  Tensor wt = wt_opt.has_value() ? *wt_opt : w.t();  // no W'^T: only the shape checks use the view
  if (wt_opt.has_value())
    TORCH_CHECK(wt.dim() == 2 && wt.stride(1) == 1 && wt.scalar_type() == at::kBFloat16 && wt.stride(0) % 8 == 0,
                "lora_refresh: bf16 W'^T");
  grt::LoraRefreshParams p{};
  p.ntarget = (int)bs.size();
  p.r = (int)bs[0].size(1);
  TORCH_CHECK(p.r % 64 == 0 && col0 % 8 == 0 && w.stride(0) % 8 == 0, "lora_refresh: r % 64");
  for (size_t j = 0; j < bs.size(); ++j) {
    check_contig(bs[j], "B");
    TORCH_CHECK(bs[j].scalar_type() == at::kBFloat16 && bs[j].size(1) == p.r && bs[j].size(0) % 64 == 0 &&
                    offs[j] % 8 == 0 && offs[j] + bs[j].size(0) <= w.size(0) &&
                    col0 + (int64_t)(j + 1) * p.r <= w.size(1) && wt_row0 + (int64_t)(j + 1) * p.r <= wt.size(0) &&
                    (!wt_opt.has_value() || offs[j] + bs[j].size(0) <= wt.size(1)),
                "lora_refresh: B_i bf16 [n % 64 == 0, r] inside W'");
    p.b[j] = bs[j].data_ptr(); p.off[j] = (int)offs[j]; p.n[j] = (int)bs[j].size(0);
  }
  p.w = w.data_ptr(); p.ldw = w.stride(0); p.col0 = (int)col0; p.trow0 = (int)wt_row0;
  p.wt = wt_opt.has_value() ? wt.data_ptr() : nullptr;
  p.ldt = wt_opt.has_value() ? wt.stride(0) : 0;
  c10::OptionalDeviceGuard g(w.device());
  grt::lora_refresh(p, cur_stream(w));
}

// ------------------------------------------------------------------ cross entropy
std::vector<Tensor> ce_fwd(const Tensor& logits, const Tensor& labels, int64_t ignore_index) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1, "logits must be [N, V] row-major");
  check_contig(labels, "labels");
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.numel() == logits.size(0) &&
              labels.device() == logits.device(), "labels must be int64 [N] on the logits' device");
  c10::OptionalDeviceGuard g(logits.device());
  const int64_t N = logits.size(0);
  auto loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  grt::cross_entropy_fwd(dtype_of(logits), logits.data_ptr(), logits.stride(0), labels.data_ptr<int64_t>(),
                         loss.data_ptr<float>(), lse.data_ptr<float>(), N, (int)logits.size(1), ignore_index,
                         cur_stream(logits));
  return {loss, lse};
}
Tensor ce_bwd(const Tensor& logits, const Tensor& labels, const Tensor& lse, const Tensor& gscale,
              int64_t ignore_index, bool inplace) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1, "logits must be [N, V] row-major");
  check_contig(labels, "labels");
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.numel() == logits.size(0) &&
              labels.device() == logits.device(), "labels must be int64 [N] on the logits' device");
  check_contig(lse, "lse");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == logits.size(0) && lse.device() == logits.device(),
              "lse fp32 [N] on the logits' device");
  check_contig(gscale, "gscale");
  TORCH_CHECK(gscale.scalar_type() == at::kFloat && gscale.numel() == logits.size(0) &&
              gscale.device() == logits.device(), "gscale fp32 [N] on the logits' device");
  c10::OptionalDeviceGuard g(logits.device());
  Tensor d = inplace ? logits : at::empty_like(logits, at::MemoryFormat::Contiguous);
  grt::cross_entropy_bwd(dtype_of(logits), logits.data_ptr(), logits.stride(0), labels.data_ptr<int64_t>(),
                         lse.data_ptr<float>(), gscale.data_ptr<float>(), d.data_ptr(), d.stride(0),
                         logits.size(0), (int)logits.size(1), ignore_index, cur_stream(logits));
  return d;
}

// ------------------------------------------------------------------ optimizer
// The optimizer kernels size every access from p (or x) alone and read their small fp32 operands at
// fixed indices (hyper[0..9], gscale[1], ws[0..nparts), out[0..1], a_ptr[0]), so each binding checks
// every operand on the host before the launch.

// a small fp32 operand: contiguous, at least min_numel values, on the device of the tensor `on`
void check_optim_f32(const Tensor& t, const Tensor& on, int64_t min_numel, const char* name, const char* on_name) {
  check_contig(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() >= min_numel && t.device() == on.device(), name,
              " must hold at least ", min_numel, " fp32 value(s) on the device of ", on_name, " (got ", t.numel(),
              " of ", t.scalar_type(), " on ", t.device(), ")");
}
void check_optim_device(const Tensor& t, const Tensor& on, const char* name, const char* on_name) {
  TORCH_CHECK(t.device() == on.device(), name, " must be on the device of ", on_name, " (", t.device(), " vs ",
              on.device(), ")");
}
constexpr const char* kHyperDoc = "hyper (lr, b1, b2, eps, wd, bc1, bc2, gscale, stochastic_rounding, step)";

int64_t sumsq_blocks() { return grt::optim_sumsq_blocks(); }
void sumsq(const Tensor& x, Tensor& ws, int64_t slot) {
  check_contig(x, "x");
  TORCH_CHECK(slot >= 0, "sumsq: slot must be >= 0, got ", slot);
  check_optim_f32(ws, x, (slot + 1) * grt::optim_sumsq_blocks(), "sumsq: ws", "x");
  c10::OptionalDeviceGuard g(x.device());
  grt::sumsq_accumulate(dtype_of(x), x.data_ptr(), x.numel(), ws.data_ptr<float>(), (int)slot, cur_stream(x));
}
void clip_finalize(const Tensor& ws, int64_t nparts, double max_norm, double prescale, Tensor& out) {
  check_contig(ws, "ws");
  TORCH_CHECK(ws.scalar_type() == at::kFloat, "clip_finalize: ws must be fp32, got ", ws.scalar_type());
  TORCH_CHECK(nparts >= 0 && nparts <= ws.numel(), "clip_finalize: nparts ", nparts, " outside ws [", ws.numel(), "]");
  check_optim_f32(out, ws, 2, "clip_finalize: out", "ws");
  c10::OptionalDeviceGuard g(ws.device());
  grt::clip_coef_finalize(ws.data_ptr<float>(), (int)nparts, (float)max_norm, (float)prescale, out.data_ptr<float>(),
                          cur_stream(ws));
}
void adamw(Tensor& p, const Tensor& gr, Tensor& m, Tensor& v, const optional<Tensor>& master, const Tensor& hyper,
           const optional<Tensor>& gscale, int64_t max_blocks, int64_t index_offset) {
  TORCH_CHECK(index_offset >= 0 && index_offset % 4 == 0, "adamw: index_offset must be a multiple of 4");
  check_contig(p, "p");
  check_contig(gr, "g");
  check_contig(m, "m");
  check_contig(v, "v");
  const int64_t n = p.numel();
  TORCH_CHECK(gr.numel() == n && m.numel() == n && v.numel() == n, "adamw size mismatch");
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat, "adam state must be fp32");
  check_optim_device(gr, p, "adamw: g", "p");
  check_optim_device(m, p, "adamw: m", "p");
  check_optim_device(v, p, "adamw: v", "p");
  check_optim_f32(hyper, p, 10, kHyperDoc, "p");
  if (gscale.has_value()) check_optim_f32(*gscale, p, 2, "adamw: gscale ([norm, coefficient])", "p");
  for (const Tensor* t : std::initializer_list<const Tensor*>{&p, &gr, &m, &v})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0 ||
                    (t->element_size() == 2 && reinterpret_cast<uintptr_t>(t->data_ptr()) % 8 == 0),
                "adamw operands must be vector aligned");
  if (master.has_value()) {
    check_contig(*master, "master");
    TORCH_CHECK(master->numel() == n && master->scalar_type() == at::kFloat, "master fp32 [n]");
    check_optim_device(*master, p, "adamw: master", "p");
  }
  c10::OptionalDeviceGuard g(p.device());
  grt::adamw_step(dtype_of(p), dtype_of(gr), p.data_ptr(), gr.data_ptr(), m.data_ptr<float>(), v.data_ptr<float>(),
                  master.has_value() ? master->data_ptr<float>() : nullptr, n, hyper.data_ptr<float>(),
                  gscale.has_value() ? gscale->data_ptr<float>() : nullptr, cur_stream(p), (int)max_blocks,
                  index_offset);
}
// 8-bit block-quantised moments (adamw8.hip): uint8 codes [n] and fp32 absmax [ceil(n / 256)]. The
// kernels load 8 codes at a time, so code arrays are 8-byte aligned.
void check_q8_state(const Tensor& codes, const Tensor& absmax, const Tensor& on, int64_t n, const char* what) {
  check_contig(codes, what);
  check_contig(absmax, what);
  TORCH_CHECK(codes.scalar_type() == at::kByte && codes.numel() == n, what, ": codes must be uint8 [", n, "], got ",
              codes.numel(), " of ", codes.scalar_type());
  TORCH_CHECK(absmax.scalar_type() == at::kFloat && absmax.numel() == (n + 255) / 256, what,
              ": absmax must be fp32 [ceil(n / 256) = ", (n + 255) / 256, "], got ", absmax.numel(), " of ",
              absmax.scalar_type());
  check_optim_device(codes, on, what, "p");
  check_optim_device(absmax, on, what, "p");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(codes.data_ptr()) % 8 == 0, what, ": codes must be 8-byte aligned");
}
void adamw8(Tensor& p, const Tensor& gr, Tensor& codes_m, Tensor& absmax_m, Tensor& codes_v, Tensor& absmax_v,
            const optional<Tensor>& master, const Tensor& hyper, const optional<Tensor>& gscale, int64_t max_blocks,
            int64_t index_offset) {
  TORCH_CHECK(index_offset >= 0 && index_offset % 256 == 0,
              "adamw8: index_offset must be a multiple of 256 (a slice starts on a block boundary), got ", index_offset);
  check_contig(p, "p");
  check_contig(gr, "g");
  const int64_t n = p.numel();
  TORCH_CHECK(gr.numel() == n, "adamw8 size mismatch: p ", n, ", g ", gr.numel());
  const bool bf = p.scalar_type() == at::kBFloat16 && gr.scalar_type() == at::kBFloat16;
  const bool f32 = p.scalar_type() == at::kFloat && gr.scalar_type() == at::kFloat;
  TORCH_CHECK(bf || f32, "adamw8: p and g must both be bf16 or both be fp32, got ", p.scalar_type(), " and ",
              gr.scalar_type());
  check_optim_device(gr, p, "adamw8: g", "p");
  check_q8_state(codes_m, absmax_m, p, n, "adamw8: exp_avg");
  check_q8_state(codes_v, absmax_v, p, n, "adamw8: exp_avg_sq");
  check_optim_f32(hyper, p, 10, kHyperDoc, "p");
  if (gscale.has_value()) check_optim_f32(*gscale, p, 2, "adamw8: gscale ([norm, coefficient])", "p");
  for (const Tensor* t : std::initializer_list<const Tensor*>{&p, &gr})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0 ||
                    (t->element_size() == 2 && reinterpret_cast<uintptr_t>(t->data_ptr()) % 8 == 0),
                "adamw8 operands must be vector aligned");
  if (master.has_value()) {
    check_contig(*master, "master");
    TORCH_CHECK(bf, "adamw8: a master copy goes with bf16 parameters");
    TORCH_CHECK(master->numel() == n && master->scalar_type() == at::kFloat, "master fp32 [n]");
    check_optim_device(*master, p, "adamw8: master", "p");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(master->data_ptr()) % 16 == 0, "adamw8: master must be 16-byte aligned");
  }
  c10::OptionalDeviceGuard g(p.device());
  grt::adamw8_step(dtype_of(p), p.data_ptr(), gr.data_ptr(), codes_m.data_ptr<uint8_t>(), absmax_m.data_ptr<float>(),
                   codes_v.data_ptr<uint8_t>(), absmax_v.data_ptr<float>(),
                   master.has_value() ? master->data_ptr<float>() : nullptr, n, hyper.data_ptr<float>(),
                   gscale.has_value() ? gscale->data_ptr<float>() : nullptr, cur_stream(p), (int)max_blocks,
                   index_offset);
}
void quantize_blockwise8(const Tensor& x, Tensor& codes, Tensor& absmax, bool is_signed) {
  check_contig(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat, "quantize_blockwise8: x must be fp32, got ", x.scalar_type());
  check_q8_state(codes, absmax, x, x.numel(), "quantize_blockwise8");
  c10::OptionalDeviceGuard g(x.device());
  grt::quantize_blockwise8(x.data_ptr<float>(), codes.data_ptr<uint8_t>(), absmax.data_ptr<float>(), x.numel(),
                           is_signed, cur_stream(x));
}
void dequantize_blockwise8(const Tensor& codes, const Tensor& absmax, Tensor& out, bool is_signed) {
  check_contig(out, "out");
  TORCH_CHECK(out.scalar_type() == at::kFloat, "dequantize_blockwise8: out must be fp32, got ", out.scalar_type());
  check_q8_state(codes, absmax, out, out.numel(), "dequantize_blockwise8");
  c10::OptionalDeviceGuard g(out.device());
  grt::dequantize_blockwise8(codes.data_ptr<uint8_t>(), absmax.data_ptr<float>(), out.data_ptr<float>(), out.numel(),
                             is_signed, cur_stream(out));
}
// AdamW on a bf16 weight [rows, cols] that also writes pt = W^T [cols, rows] (see optim.hip)
void adamw_t(Tensor& p, const Tensor& gr, Tensor& m, Tensor& v, const Tensor& hyper, const optional<Tensor>& gscale,
             Tensor& pt, int64_t index_offset) {
  for (const Tensor* t : std::initializer_list<const Tensor*>{&p, &gr, &m, &v, &pt}) check_contig(*t, "adamw_t operand");
  TORCH_CHECK(p.dim() == 2 && p.size(0) % 64 == 0 && p.size(1) % 128 == 0, "adamw_t: rows % 64 == 0, cols % 128 == 0");
  TORCH_CHECK(p.scalar_type() == at::kBFloat16 && gr.scalar_type() == at::kBFloat16 && pt.scalar_type() == at::kBFloat16,
              "adamw_t: bf16 param / grad / transpose");
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat, "adamw_t: fp32 moments");
  TORCH_CHECK(gr.numel() == p.numel() && m.numel() == p.numel() && v.numel() == p.numel(), "adamw_t: sizes");
  TORCH_CHECK(pt.dim() == 2 && pt.size(0) == p.size(1) && pt.size(1) == p.size(0), "adamw_t: pt must be [cols, rows]");
  for (const Tensor* t : std::initializer_list<const Tensor*>{&gr, &m, &v, &pt})
    check_optim_device(*t, p, "adamw_t: g / m / v / pt", "p");
  check_optim_f32(hyper, p, 10, kHyperDoc, "p");
  if (gscale.has_value()) check_optim_f32(*gscale, p, 2, "adamw_t: gscale ([norm, coefficient])", "p");
  TORCH_CHECK(index_offset >= 0 && index_offset % 4 == 0, "adamw_t: index_offset must be a multiple of 4");
  for (const Tensor* t : std::initializer_list<const Tensor*>{&p, &gr, &m, &v, &pt})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "adamw_t operands must be 16-byte aligned");
  c10::OptionalDeviceGuard g(p.device());
  grt::adamw_t_step(p.data_ptr(), gr.data_ptr(), m.data_ptr<float>(), v.data_ptr<float>(), pt.data_ptr(), p.size(0),
                    p.size(1), hyper.data_ptr<float>(), gscale.has_value() ? gscale->data_ptr<float>() : nullptr,
                    cur_stream(p), index_offset);
}

void scale_(Tensor& x, double a, const optional<Tensor>& a_ptr) {
  check_contig(x, "x");
  if (a_ptr.has_value()) check_optim_f32(*a_ptr, x, 1, "scale_: a_ptr", "x");
  c10::OptionalDeviceGuard g(x.device());
  grt::scale_inplace(dtype_of(x), x.data_ptr(), x.numel(), (float)a,
                     a_ptr.has_value() ? a_ptr->data_ptr<float>() : nullptr, cur_stream(x));
}

// ------------------------------------------------------------------ attention
void check_bshd(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.dim() == 4, name, " must be [B, S, H, D]");
  TORCH_CHECK(t.stride(3) == 1, name, ": head_dim must be contiguous");
  if (t.scalar_type() == at::kBFloat16) {
    TORCH_CHECK(grt::attn_bf16_supported((int)t.size(3)), name, ": bf16 kernels need head_dim 64 or 128");
  } else {
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be bf16 or fp32");
    TORCH_CHECK(grt::attn_f32_supported((int)t.size(3)), name, ": fp32 kernels need head_dim 64 or 128");
  }
  const int64_t vec = 16 / t.element_size();
  TORCH_CHECK(t.stride(0) % vec == 0 && t.stride(1) % vec == 0 && t.stride(2) % vec == 0 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, ": strides must keep 16-byte alignment");
}

grt::AttnParams make_params(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o, Tensor& lse,
                            double scale, bool causal, const optional<Tensor>& seqlens_k,
                            const optional<Tensor>& cu_seqlens = {}, int64_t max_seqlen = 0) {
  check_bshd(q, "q");
  check_bshd(k, "k");
  check_bshd(v, "v");
  check_bshd(o, "o");
  TORCH_CHECK(k.sizes() == v.sizes(), "k/v shape mismatch");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type() &&
                  o.scalar_type() == q.scalar_type(), "q/k/v/o dtype mismatch");
  TORCH_CHECK(k.size(3) == q.size(3), "head_dim mismatch");
  TORCH_CHECK(q.size(0) == k.size(0) && o.sizes() == q.sizes(), "batch/out shape mismatch");
  TORCH_CHECK(q.size(2) % k.size(2) == 0, "Hq must be a multiple of Hkv");
  const bool packed = cu_seqlens.has_value();
  const int64_t nseq = packed ? cu_seqlens->numel() - 1 : q.size(0);
  const int64_t sq_rows = packed ? max_seqlen : q.size(1);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == nseq * q.size(2) * sq_rows,
              "lse must be fp32 [B, Hq, Sq] ([num_seqs, Hq, max_seqlen] when packed)");
  grt::AttnParams p{};
  p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = o.data_ptr(); p.lse = lse.data_ptr<float>();
  p.q_bs = q.stride(0); p.q_ss = q.stride(1); p.q_hs = q.stride(2);
  p.k_bs = k.stride(0); p.k_ss = k.stride(1); p.k_hs = k.stride(2);
  p.v_bs = v.stride(0); p.v_ss = v.stride(1); p.v_hs = v.stride(2);
  p.o_bs = o.stride(0); p.o_ss = o.stride(1); p.o_hs = o.stride(2);
  p.B = (int)q.size(0); p.Sq = (int)q.size(1); p.Sk = (int)k.size(1);
  p.Hq = (int)q.size(2); p.Hkv = (int)k.size(2); p.D = (int)q.size(3);
  p.scale = (float)scale;
  p.causal = causal ? 1 : 0;
  if (causal) TORCH_CHECK(p.Sk >= p.Sq, "causal attention needs Sk >= Sq");
  p.seqlens_k = nullptr;
  if (seqlens_k.has_value()) {
    check_contig(*seqlens_k, "seqlens_k");
    TORCH_CHECK(seqlens_k->scalar_type() == at::kInt && seqlens_k->numel() == q.size(0), "seqlens_k int32 [B]");
    p.seqlens_k = seqlens_k->data_ptr<int32_t>();
  }
  p.cu_seqlens = nullptr;
  if (packed) {  // padding-free: [1, T, H, D] tensors, sequence b = token rows [cu[b], cu[b+1])
    check_contig(*cu_seqlens, "cu_seqlens");
    TORCH_CHECK(cu_seqlens->scalar_type() == at::kInt && cu_seqlens->is_cuda() && nseq >= 1,
                "cu_seqlens must be int32 [num_seqs + 1] on the device");
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && q.size(3) == 128,
                "packed (cu_seqlens) attention: bf16 kernels, head_dim 128");
    TORCH_CHECK(q.size(0) == 1 && k.size(1) == q.size(1), "packed attention: q / k / v are [1, T, H, D]");
    TORCH_CHECK(causal && !seqlens_k.has_value(), "packed attention is causal self-attention without seqlens_k");
    TORCH_CHECK(max_seqlen >= 1 && max_seqlen <= q.size(1), "max_seqlen must be in [1, T]");
    p.cu_seqlens = cu_seqlens->data_ptr<int32_t>();
    p.B = (int)nseq;
    p.Sq = p.Sk = (int)max_seqlen;
    p.q_bs = p.k_bs = p.v_bs = p.o_bs = 0;
  }
  p.drop_seed = 0;
  p.drop_thresh = 0;
  p.drop_scale = 1.f;
  return p;
}

void set_dropout(grt::AttnParams& p, double dropout_p, int64_t seed) {
  TORCH_CHECK(dropout_p >= 0.0 && dropout_p < 1.0, "attention dropout p must be in [0, 1)");
  if (dropout_p <= 0.0) return;
  p.drop_seed = (uint32_t)(seed & 0xffffffffLL);
  p.drop_thresh = (uint32_t)std::min(4294967295.0, std::ceil(dropout_p * 4294967296.0));
  if (p.drop_thresh == 0) p.drop_thresh = 1;
  p.drop_scale = (float)(1.0 / (1.0 - dropout_p));
}

std::vector<Tensor> attn_fwd(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& out,
                             double scale, bool causal, const optional<Tensor>& seqlens_k, double dropout_p,
                             int64_t seed, const optional<Tensor>& cu_seqlens, int64_t max_seqlen,
                             const optional<Tensor>& o_t) {
  c10::OptionalDeviceGuard g(q.device());
  Tensor o = out.has_value() ? *out : at::empty(q.sizes(), q.options());
  auto lse = cu_seqlens.has_value()
                 ? at::empty({cu_seqlens->numel() - 1, q.size(2), max_seqlen}, q.options().dtype(at::kFloat))
                 : at::empty({q.size(0), q.size(2), q.size(1)}, q.options().dtype(at::kFloat));
  auto p = make_params(q, k, v, o, lse, scale, causal, seqlens_k, cu_seqlens, max_seqlen);
  set_dropout(p, dropout_p, seed);
  if (o_t.has_value()) {  // transposed output [Hq * D, B * S] beside o (o projection's weight gradient)
    check_contig(*o_t, "o_t");
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && p.D == 128 && o_t->scalar_type() == at::kBFloat16 &&
                    o_t->dim() == 2 && o_t->size(0) == (int64_t)p.Hq * p.D && o_t->size(1) == q.size(0) * q.size(1),
                "attn_fwd o_t: bf16, head_dim 128, shape [Hq * D, B * S]");
    p.o_t = o_t->data_ptr();
    p.ot_ld = o_t->size(1);
  }
  if (q.scalar_type() == at::kFloat) grt::attn_fwd_f32(p, cur_stream(q));
  else if (p.D == 64) grt::attn_fwd_d64(p, cur_stream(q));
  else grt::attn_fwd(p, cur_stream(q));
  return {o, lse};
}

std::vector<Tensor> attn_bwd(const Tensor& dout, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& o,
                             Tensor& lse, const optional<Tensor>& dq_out, const optional<Tensor>& dk_out,
                             const optional<Tensor>& dv_out, double scale, bool causal,
                             const optional<Tensor>& seqlens_k, double dropout_p, int64_t seed,
                             const optional<Tensor>& rope_cos, const optional<Tensor>& rope_sin,
                             const optional<Tensor>& cu_seqlens, int64_t max_seqlen, const optional<Tensor>& dqkv_t) {
  c10::OptionalDeviceGuard g(q.device());
  check_bshd(dout, "dout");
  TORCH_CHECK(dout.sizes() == q.sizes(), "dout shape");
  auto p = make_params(q, k, v, o, lse, scale, causal, seqlens_k, cu_seqlens, max_seqlen);
  set_dropout(p, dropout_p, seed);
  Tensor dq = dq_out.has_value() ? *dq_out : at::empty(q.sizes(), q.options());
  Tensor dk = dk_out.has_value() ? *dk_out : at::empty(k.sizes(), k.options());
  Tensor dv = dv_out.has_value() ? *dv_out : at::empty(v.sizes(), v.options());
  check_bshd(dq, "dq");
  check_bshd(dk, "dk");
  check_bshd(dv, "dv");
  TORCH_CHECK(dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == v.sizes(), "grad shapes");
  auto ws = at::empty({grt::attn_bwd_workspace_floats(p.B, p.Hq, p.Sq, p.D)}, q.options().dtype(at::kFloat));
  grt::AttnBwdParams bp{};
  bp.f = p;
  bp.dout = dout.data_ptr(); bp.do_bs = dout.stride(0); bp.do_ss = dout.stride(1); bp.do_hs = dout.stride(2);
  bp.dq = dq.data_ptr(); bp.dq_bs = dq.stride(0); bp.dq_ss = dq.stride(1); bp.dq_hs = dq.stride(2);
  bp.dk = dk.data_ptr(); bp.dk_bs = dk.stride(0); bp.dk_ss = dk.stride(1); bp.dk_hs = dk.stride(2);
  bp.dv = dv.data_ptr(); bp.dv_bs = dv.stride(0); bp.dv_ss = dv.stride(1); bp.dv_hs = dv.stride(2);
  if (cu_seqlens.has_value()) bp.do_bs = bp.dq_bs = bp.dk_bs = bp.dv_bs = 0;  // packed: one token axis
  bp.delta = ws.data_ptr<float>();
  TORCH_CHECK(rope_cos.has_value() == rope_sin.has_value(), "attn_bwd: rope_cos and rope_sin together");
  if (rope_cos.has_value()) {  // dQ / dK written un-rotated (q / k were rotated at position = index)
    check_contig(*rope_cos, "rope_cos");
    check_contig(*rope_sin, "rope_sin");
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && p.D == 128, "attn_bwd rope epilogue: bf16, head_dim 128");
    TORCH_CHECK(rope_cos->scalar_type() == at::kFloat && rope_sin->sizes() == rope_cos->sizes() &&
                    rope_sin->scalar_type() == at::kFloat && rope_cos->dim() == 2 && rope_cos->size(1) == p.D / 2 &&
                    rope_cos->size(0) >= std::max(p.Sq, p.Sk),
                "attn_bwd: rope tables fp32 [>= max(Sq, Sk), D / 2]");
    bp.rope_cos = rope_cos->data_ptr<float>();
    bp.rope_sin = rope_sin->data_ptr<float>();
  }
  TORCH_CHECK(dout.scalar_type() == q.scalar_type() && dq.scalar_type() == q.scalar_type() &&
                  dk.scalar_type() == q.scalar_type() && dv.scalar_type() == q.scalar_type(), "grad dtype mismatch");
  if (dqkv_t.has_value()) {  // transposed fused-QKV gradient [(Hq + 2 Hkv) D, B * S] beside dq / dk / dv
    check_contig(*dqkv_t, "dqkv_t");
    TORCH_CHECK(q.scalar_type() == at::kBFloat16 && p.D == 128 && dqkv_t->scalar_type() == at::kBFloat16,
                "attn_bwd dqkv_t: bf16, head_dim 128");
    TORCH_CHECK(p.Sq == p.Sk && dqkv_t->dim() == 2 && dqkv_t->size(0) == (int64_t)(p.Hq + 2 * p.Hkv) * p.D &&
                    dqkv_t->size(1) == q.size(0) * q.size(1),
                "attn_bwd dqkv_t: self-attention, shape [(Hq + 2 Hkv) * D, B * S]");
    bp.dqkv_t = dqkv_t->data_ptr();
    bp.t_ld = dqkv_t->size(1);
    bp.t_row_q = 0;
    bp.t_row_k = p.Hq * p.D;
    bp.t_row_v = (p.Hq + p.Hkv) * p.D;
  }
  if (q.scalar_type() == at::kFloat) grt::attn_bwd_f32(bp, cur_stream(q));
  else if (p.D == 64) grt::attn_bwd_d64(bp, cur_stream(q));
  else grt::attn_bwd(bp, cur_stream(q));
  return {dq, dk, dv};
}

// ---- RoPE + attention on the fused QKV buffer, bf16 head_dim 64 (attention_d64.hip, FusedRope policy) ----
// row stride of t seen as T token rows of Hq heads: [T, Hq * 64] or [T, Hq, 64] with unit last stride and
// heads 64 apart; the rows may be the head of a wider row buffer
int64_t d64_row_stride(const Tensor& t, int64_t T, int64_t hq, const char* op, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", name, " must be bf16");
  const bool ok = t.dim() == 2 ? t.size(0) == T && t.size(1) == hq * 64 && t.stride(1) == 1
                               : t.dim() == 3 && t.size(0) == T && t.size(1) == hq && t.size(2) == 64 &&
                                     t.stride(2) == 1 && (hq == 1 || t.stride(1) == 64);
  const int64_t ld = ok && T > 1 ? t.stride(0) : hq * 64;  // one row: its stride is never used
  TORCH_CHECK(ok && ld >= hq * 64, op, ": ", name, " must be [T, Hq * 64] or [T, Hq, 64] token rows (unit last stride, "
              "heads 64 apart, row stride >= Hq * 64)");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", name, " alignment");
  return ld;
}

grt::RopeAttnD64Params rope_attn_d64_params(const char* op, const Tensor& qkv, const Tensor& cos, const Tensor& sin,
                                            const Tensor& o, int64_t B, int64_t S, int64_t hq, int64_t hkv,
                                            double scale, bool causal, const optional<Tensor>& cu_seqlens,
                                            int64_t max_seqlen) {
  check_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, op, ": qkv must be bf16, got ", qkv.scalar_type());
  TORCH_CHECK(qkv.dim() == 2 && qkv.is_contiguous(), op, ": qkv must be a contiguous [T, (Hq + 2 Hkv) * 64]");
  TORCH_CHECK(hq >= 1 && hkv >= 1 && hq % hkv == 0, op, ": Hq must be a multiple of Hkv");
  TORCH_CHECK(qkv.size(1) == (hq + 2 * hkv) * 64, op, ": qkv width ", qkv.size(1), " is not (Hq + 2 Hkv) * 64 = ",
              (hq + 2 * hkv) * 64);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, op, ": qkv alignment");
  const int64_t T = qkv.size(0);
  TORCH_CHECK(B >= 1 && S >= 1 && B * S == T, op, ": B * S must equal the token rows of qkv");
  const bool packed = cu_seqlens.has_value();
  const int64_t rows = packed ? max_seqlen : S;  // longest sequence = positions the tables must cover
  int64_t nseq = B;
  if (packed) {
    TORCH_CHECK(cu_seqlens->is_cuda() && cu_seqlens->scalar_type() == at::kInt && cu_seqlens->is_contiguous() &&
                    cu_seqlens->dim() == 1 && cu_seqlens->numel() >= 2,
                op, ": cu_seqlens must be int32 [num_seqs + 1] on the device");
    TORCH_CHECK(max_seqlen >= 1 && max_seqlen <= T, op, ": max_seqlen must be in [1, T]");
    nseq = cu_seqlens->numel() - 1;
  }
  check_contig(cos, "cos");
  check_contig(sin, "sin");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat, op, ": cos/sin must be fp32");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 32 && sin.sizes() == cos.sizes(), op, ": cos/sin must be [rows, 32]");
  TORCH_CHECK(cos.size(0) >= rows, op, ": cos/sin tables have ", cos.size(0), " rows, the longest sequence has ", rows);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(cos.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(sin.data_ptr()) % 16 == 0,
              op, ": cos/sin alignment");
  TORCH_CHECK(nseq * hq * rows < INT_MAX / 64 && T < INT_MAX, op, ": problem too large");
  grt::RopeAttnD64Params p{};
  p.qkv = qkv.data_ptr(); p.ld = qkv.size(1);
  p.cos = cos.data_ptr<float>(); p.sin = sin.data_ptr<float>();
  p.o = o.data_ptr(); p.o_ld = d64_row_stride(o, T, hq, op, "o");
  p.cu_seqlens = packed ? cu_seqlens->data_ptr<int32_t>() : nullptr;
  p.T = T; p.nseq = (int)nseq; p.S = (int)rows; p.Hq = (int)hq; p.Hkv = (int)hkv;
  p.scale = (float)scale; p.causal = causal ? 1 : 0;
  return p;
}

// o: [T, Hq, 64] token rows to write (may be the head of wider rows); returns lse fp32 [nseq, Hq, S]
Tensor rope_attn_fwd_d64(const Tensor& qkv, const Tensor& cos, const Tensor& sin, Tensor& o, int64_t B, int64_t S,
                         int64_t hq, int64_t hkv, double scale, bool causal, const optional<Tensor>& cu_seqlens,
                         int64_t max_seqlen) {
  auto p = rope_attn_d64_params("rope_attn_fwd_d64", qkv, cos, sin, o, B, S, hq, hkv, scale, causal, cu_seqlens,
                                max_seqlen);
  c10::OptionalDeviceGuard g(qkv.device());
  auto lse = at::empty({(int64_t)p.nseq, hq, (int64_t)p.S}, qkv.options().dtype(at::kFloat));
  p.lse = lse.data_ptr<float>();
  grt::rope_attn_fwd_d64(p, cur_stream(qkv));
  return lse;
}

// writes every element of dqkv [T, (Hq + 2 Hkv) * 64]: un-rotated dQ / dK and dV in their columns
void rope_attn_bwd_d64(const Tensor& dout, const Tensor& qkv, const Tensor& cos, const Tensor& sin, const Tensor& o,
                       const Tensor& lse, Tensor& dqkv, int64_t B, int64_t S, int64_t hq, int64_t hkv, double scale,
                       bool causal, const optional<Tensor>& cu_seqlens, int64_t max_seqlen) {
  const char* op = "rope_attn_bwd_d64";
  auto p = rope_attn_d64_params(op, qkv, cos, sin, o, B, S, hq, hkv, scale, causal, cu_seqlens, max_seqlen);
  c10::OptionalDeviceGuard g(qkv.device());
  check_cuda(lse, "lse");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == (int64_t)p.nseq * hq * p.S,
              op, ": lse must be fp32 [B, Hq, S] ([num_seqs, Hq, max_seqlen] when packed)");
  check_cuda(dqkv, "dqkv");
  TORCH_CHECK(dqkv.scalar_type() == at::kBFloat16 && dqkv.is_contiguous() && dqkv.sizes() == qkv.sizes() &&
                  reinterpret_cast<uintptr_t>(dqkv.data_ptr()) % 16 == 0,
              op, ": dqkv must be a contiguous bf16 tensor of qkv's shape");
  p.lse = const_cast<float*>(lse.data_ptr<float>());
  p.dout = dout.data_ptr(); p.do_ld = d64_row_stride(dout, p.T, hq, op, "do");
  p.dqkv = dqkv.data_ptr();
  auto ws = at::empty({(int64_t)p.nseq * hq * p.S}, qkv.options().dtype(at::kFloat));
  p.delta = ws.data_ptr<float>();
  grt::rope_attn_bwd_d64(p, cur_stream(qkv));
}

// Split-K decode attention (decode_attention.hip). D is the binding's head dim: attn_decode is the
// head_dim-128 binding and refuses anything else, attn_decode_d64 the head_dim-64 one; multi: T 2..4.
Tensor attn_decode_impl(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& seqlens_k,
                        double scale, int64_t D, const char* op, std::vector<Tensor>* partials = nullptr,
                        bool multi = false) {
  check_bshd(q, "q");
  check_bshd(k, "k");
  check_bshd(v, "v");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16,
              op, ": bf16");
  TORCH_CHECK(q.size(3) == D && k.size(3) == D && v.size(3) == D, op, ": head_dim ", D);
  if (multi) {
    TORCH_CHECK(q.size(1) >= 2 && q.size(1) <= 4, op, ": 2 to 4 query tokens per sequence, got ", q.size(1));
  } else {
    TORCH_CHECK(q.size(1) == 1, op, ": one query token per sequence");
  }
  const int64_t T = q.size(1);
  TORCH_CHECK(k.sizes() == v.sizes() && k.size(0) == q.size(0), op, ": k/v shapes");
  const int64_t Hq = q.size(2), Hkv = k.size(2);
  TORCH_CHECK(Hq % Hkv == 0, op, ": Hq % Hkv");
  const int64_t G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, op, ": GQA group must be 1, 2, 4 or 8");
  if (D == 64 || multi) {
    // the kernel reads q / k / v with 16-byte loads at any (batch, key, head) offset
    for (const Tensor* t : {&q, &k, &v}) {
      TORCH_CHECK(t->device() == q.device(), op, ": q / k / v on one device");
      TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 && t->stride(2) % 8 == 0 && t->stride(3) == 1,
                  op, ": every stride a multiple of 8 elements, unit head_dim stride");
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, op, ": 16-byte aligned base pointers");
    }
    TORCH_CHECK(k.size(1) <= INT32_MAX && q.size(0) * T * Hq <= INT32_MAX, op, ": dims");
  }
  c10::OptionalDeviceGuard g(q.device());
  grt::AttnDecodeParams p{};
  p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr();
  auto o = at::empty(q.sizes(), q.options());
  p.o = o.data_ptr();
  p.q_bs = q.stride(0); p.q_hs = q.stride(2);
  p.k_bs = k.stride(0); p.k_ss = k.stride(1); p.k_hs = k.stride(2);
  p.v_bs = v.stride(0); p.v_ss = v.stride(1); p.v_hs = v.stride(2);
  p.o_bs = o.stride(0); p.o_hs = o.stride(2);
  p.T = (int)T; p.q_ts = q.stride(1); p.o_ts = o.stride(1);
  p.B = (int)q.size(0); p.Hq = (int)Hq; p.Hkv = (int)Hkv; p.Sk = (int)k.size(1);
  p.NS = grt::attn_decode_splits(p.B, p.Hkv, p.Sk, (int)D);
  p.seqlens_k = nullptr;
  if (seqlens_k.has_value()) {
    check_contig(*seqlens_k, "seqlens_k");
    TORCH_CHECK(seqlens_k->scalar_type() == at::kInt && seqlens_k->numel() == q.size(0), "seqlens_k int32 [B]");
    if (D == 64 || multi) TORCH_CHECK(seqlens_k->device() == q.device(), op, ": seqlens_k on q's device");
    p.seqlens_k = seqlens_k->data_ptr<int32_t>();
  }
  p.scale_log2 = (float)(scale * 1.4426950408889634);
  const int64_t rows = (int64_t)p.B * T * Hq;  // [B, T, Hq] partial states per split
  auto ws = at::empty({rows * p.NS * (D + 2)}, q.options().dtype(at::kFloat));
  p.part_o = ws.data_ptr<float>();
  p.part_m = p.part_o + rows * p.NS * D;
  p.part_l = p.part_m + rows * p.NS;
  grt::attn_decode(p, (int)D, cur_stream(q));
  if (partials) {
    const int64_t n = rows * p.NS;
    *partials = {ws.narrow(0, 0, n * D).view({p.B, Hq, p.NS, D}), ws.narrow(0, n * D, n).view({p.B, Hq, p.NS}),
                 ws.narrow(0, n * D + n, n).view({p.B, Hq, p.NS})};
  }
  return o;
}

Tensor attn_decode(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& seqlens_k, double scale) {
  return attn_decode_impl(q, k, v, seqlens_k, scale, 128, "attn_decode");
}

Tensor attn_decode_d64(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& seqlens_k,
                       double scale) {
  return attn_decode_impl(q, k, v, seqlens_k, scale, 64, "attn_decode_d64");
}

// Verify step of speculative decoding: q [B, T, Hq, D], T in 2..4, whose keys are the last T of each
// row; token t attends keys [0, seqlens_k[b] - (T - 1 - t)) (seqlens_k absent: all Sk keys are valid).
Tensor attn_decode_multi(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& seqlens_k,
                         double scale) {
  return attn_decode_impl(q, k, v, seqlens_k, scale, 128, "attn_decode_multi", nullptr, true);
}

Tensor attn_decode_multi_d64(const Tensor& q, const Tensor& k, const Tensor& v, const optional<Tensor>& seqlens_k,
                             double scale) {
  return attn_decode_impl(q, k, v, seqlens_k, scale, 64, "attn_decode_multi_d64", nullptr, true);
}

// Decode attention over an fp8 cache (attn_decode_split_kernel with uint8 cache elements): q bf16
// [B, T, Hq, D], T in 1..4; k / v codes with their scales; same split plan and token rule as above.
Tensor attn_decode_fp8_impl(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& k_scale,
                            const Tensor& v_scale, const optional<Tensor>& seqlens_k, double scale, int64_t D,
                            const char* op) {
  check_cuda(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.scalar_type() == at::kBFloat16 && q.stride(3) == 1, op, ": q must be bf16 [B, T, Hq, D]");
  check_fp8_cache(k, k_scale, q, op, "k");
  check_fp8_cache(v, v_scale, q, op, "v");
  TORCH_CHECK(q.size(3) == D && k.size(3) == D && v.size(3) == D, op, ": head_dim ", D);
  const int64_t T = q.size(1);
  TORCH_CHECK(T >= 1 && T <= 4, op, ": 1 to 4 query tokens per sequence, got ", T);
  TORCH_CHECK(k.sizes() == v.sizes() && k.size(0) == q.size(0), op, ": k/v shapes");
  const int64_t Hq = q.size(2), Hkv = k.size(2);
  TORCH_CHECK(Hq % Hkv == 0, op, ": Hq % Hkv");
  const int64_t G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, op, ": GQA group must be 1, 2, 4 or 8");
  TORCH_CHECK(q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0 && q.stride(2) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              op, ": q strides must keep 16-byte alignment");
  TORCH_CHECK(k.size(1) >= 1 && k.size(1) <= INT32_MAX && q.size(0) * T * Hq <= INT32_MAX, op, ": dims");
  c10::OptionalDeviceGuard g(q.device());
  grt::AttnDecodeParams p{};
  p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr();
  p.k_scale = k_scale.data_ptr<float>(); p.v_scale = v_scale.data_ptr<float>();
  auto o = at::empty(q.sizes(), q.options());
  p.o = o.data_ptr();
  p.q_bs = q.stride(0); p.q_hs = q.stride(2);
  p.k_bs = k.stride(0); p.k_ss = k.stride(1); p.k_hs = k.stride(2);
  p.v_bs = v.stride(0); p.v_ss = v.stride(1); p.v_hs = v.stride(2);
  p.ksc_bs = k_scale.stride(0); p.ksc_ss = k_scale.stride(1); p.ksc_hs = k_scale.stride(2);
  p.vsc_bs = v_scale.stride(0); p.vsc_ss = v_scale.stride(1); p.vsc_hs = v_scale.stride(2);
  p.o_bs = o.stride(0); p.o_hs = o.stride(2);
  p.T = (int)T; p.q_ts = q.stride(1); p.o_ts = o.stride(1);
  p.B = (int)q.size(0); p.Hq = (int)Hq; p.Hkv = (int)Hkv; p.Sk = (int)k.size(1);
  p.NS = grt::attn_decode_splits(p.B, p.Hkv, p.Sk, (int)D);
  p.seqlens_k = nullptr;
  if (seqlens_k.has_value()) {
    check_contig(*seqlens_k, "seqlens_k");
    TORCH_CHECK(seqlens_k->scalar_type() == at::kInt && seqlens_k->numel() == q.size(0) &&
                    seqlens_k->device() == q.device(),
                op, ": seqlens_k int32 [B] on q's device");
    p.seqlens_k = seqlens_k->data_ptr<int32_t>();
  }
  p.scale_log2 = (float)(scale * 1.4426950408889634);
  const int64_t rows = (int64_t)p.B * T * Hq;
  auto ws = at::empty({rows * p.NS * (D + 2)}, q.options().dtype(at::kFloat));
  p.part_o = ws.data_ptr<float>();
  p.part_m = p.part_o + rows * p.NS * D;
  p.part_l = p.part_m + rows * p.NS;
  grt::attn_decode_fp8(p, (int)D, cur_stream(q));
  return o;
}

Tensor attn_decode_fp8(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& k_scale, const Tensor& v_scale,
                       const optional<Tensor>& seqlens_k, double scale) {
  return attn_decode_fp8_impl(q, k, v, k_scale, v_scale, seqlens_k, scale, 128, "attn_decode_fp8");
}

Tensor attn_decode_fp8_d64(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& k_scale,
                           const Tensor& v_scale, const optional<Tensor>& seqlens_k, double scale) {
  return attn_decode_fp8_impl(q, k, v, k_scale, v_scale, seqlens_k, scale, 64, "attn_decode_fp8_d64");
}

// test support: attn_decode_d64 plus its per-split partial states, [o, part_o [B, Hq, NS, 64],
// part_m [B, Hq, NS] (log2 units), part_l [B, Hq, NS]]; the partials are written only when NS > 1
std::vector<Tensor> attn_decode_d64_partials(const Tensor& q, const Tensor& k, const Tensor& v,
                                             const optional<Tensor>& seqlens_k, double scale) {
  std::vector<Tensor> parts;
  Tensor o = attn_decode_impl(q, k, v, seqlens_k, scale, 64, "attn_decode_d64", &parts);
  parts.insert(parts.begin(), o);
  return parts;
}

// ------------------------------------------------------------------ NF4
std::vector<Tensor> nf4_quantize(const Tensor& w, int64_t blocksize) {
  check_contig(w, "w");
  c10::OptionalDeviceGuard g(w.device());
  const int64_t n = w.numel();
  TORCH_CHECK(n % blocksize == 0 && (blocksize == 32 || blocksize == 64 || blocksize == 128),
              "numel must be a multiple of blocksize (32/64/128)");
  auto q = at::empty({n / 2}, w.options().dtype(at::kByte));
  auto absmax = at::empty({n / blocksize}, w.options().dtype(at::kFloat));
  grt::nf4_quantize(dtype_of(w), w.data_ptr(), q.data_ptr<uint8_t>(), absmax.data_ptr<float>(), n, (int)blocksize,
                    cur_stream(w));
  return {q, absmax};
}
Tensor nf4_dequantize(const Tensor& q, const Tensor& absmax, int64_t n, int64_t blocksize, at::ScalarType dt,
                      const optional<Tensor>& out) {
  check_contig(q, "q");
  check_contig(absmax, "absmax");
  c10::OptionalDeviceGuard g(q.device());
  TORCH_CHECK(q.numel() * 2 == n && absmax.numel() * blocksize == n, "nf4 shapes");
  Tensor w = out.has_value() ? *out : at::empty({n}, q.options().dtype(dt));
  TORCH_CHECK(w.numel() == n && w.is_contiguous(), "out shape");
  grt::nf4_dequantize(dtype_of(w), q.data_ptr<uint8_t>(), absmax.data_ptr<float>(), w.data_ptr(), n, (int)blocksize,
                      cur_stream(q));
  return w;
}

// dequantise into out ([rows, cols] bf16 view, unit column stride, any row stride: the W head of a
// K-concatenated [W | B] buffer); false when the shape is not handled
bool nf4_dequantize_into(const Tensor& q, const Tensor& absmax, Tensor out, int64_t blocksize) {
  check_contig(q, "q");
  check_contig(absmax, "absmax");
  TORCH_CHECK(out.dim() == 2 && out.scalar_type() == at::kBFloat16 && out.stride(1) == 1 && out.is_cuda(),
              "nf4_dequantize_into: out must be a 2-D bf16 view with unit column stride");
  const int64_t rows = out.size(0), cols = out.size(1);
  TORCH_CHECK(q.numel() * 2 == rows * cols && absmax.numel() * blocksize == rows * cols, "nf4 shapes");
  TORCH_CHECK(rows <= INT32_MAX && cols <= INT32_MAX, "nf4_dequantize_into: dims");
  if (out.stride(0) % 8 != 0 || reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 != 0) return false;  // 16-byte stores
  c10::OptionalDeviceGuard g(q.device());
  return grt::nf4_dequantize_2d(q.data_ptr<uint8_t>(), absmax.data_ptr<float>(), out.data_ptr(), (int)rows,
                                (int)cols, out.stride(0), (int)blocksize, cur_stream(q));
}

Tensor nf4_dequantize_t(const Tensor& q, const Tensor& absmax, int64_t rows, int64_t cols, int64_t blocksize) {
  check_contig(q, "q");
  check_contig(absmax, "absmax");
  TORCH_CHECK(blocksize == 64 && cols % 64 == 0, "nf4_dequantize_t: blocksize 64 and cols % 64 == 0");
  TORCH_CHECK(q.numel() * 2 == rows * cols && absmax.numel() * blocksize == rows * cols, "nf4 shapes");
  TORCH_CHECK(rows <= INT32_MAX && cols <= INT32_MAX, "nf4_dequantize_t: dims");
  c10::OptionalDeviceGuard g(q.device());
  Tensor wt = at::empty({cols, rows}, q.options().dtype(at::kBFloat16));
  grt::nf4_dequantize_t(q.data_ptr<uint8_t>(), absmax.data_ptr<float>(), wt.data_ptr(), (int)rows, (int)cols,
                        (int)blocksize, cur_stream(q));
  return wt;
}

void transpose_into(const Tensor& src, Tensor& dst) {
  check_contig(src, "src");
  check_contig(dst, "dst");
  TORCH_CHECK(src.dim() == 2 && dst.dim() == 2 && src.scalar_type() == at::kBFloat16 &&
                  dst.scalar_type() == at::kBFloat16, "transpose: 2-D bf16");
  const int64_t R = src.size(0), Cc = src.size(1);
  TORCH_CHECK(dst.size(0) == Cc && dst.size(1) == R, "transpose: dst must be [cols, rows]");
  TORCH_CHECK(R % 64 == 0 && Cc % 64 == 0 && R <= INT32_MAX && Cc <= INT32_MAX, "transpose: dims must be multiples of 64");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(dst.data_ptr()) % 16 == 0,
              "transpose: 16-byte alignment");
  c10::OptionalDeviceGuard g(src.device());
  grt::transpose_bf16(src.data_ptr(), dst.data_ptr(), (int)R, (int)Cc, cur_stream(src));
}

// dst <- src (same byte count, contiguous) on the GPU tensor's current stream by a DMA (SDMA)
// engine, never by a blit kernel on the compute units: hipMemcpyDeviceToDeviceNoCU with the pointers
// as they are (a pinned host tensor is addressed through its device mapping). The offloaded
// optimizer's device -> host moment write-backs otherwise run as ROCclr __amd_rocclr_copyBuffer
// kernels beside the step's compute (profiles/r5_offload70.md).
void copy_sdma(Tensor& dst, const Tensor& src) {
  TORCH_CHECK(dst.is_contiguous() && src.is_contiguous(), "copy_sdma: contiguous tensors");
  const int64_t n = dst.numel() * dst.element_size();
  TORCH_CHECK(n == src.numel() * src.element_size(), "copy_sdma: byte counts differ");
  TORCH_CHECK(dst.is_cuda() || src.is_cuda(), "copy_sdma: one side must be a GPU tensor");
  TORCH_CHECK((dst.is_cuda() || dst.is_pinned()) && (src.is_cuda() || src.is_pinned()),
              "copy_sdma: host tensors must be pinned");
  if (n == 0) return;
  const Tensor& g = dst.is_cuda() ? dst : src;
  c10::OptionalDeviceGuard guard(g.device());
  const hipError_t e = hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), (size_t)n, hipMemcpyDeviceToDeviceNoCU,
                                      cur_stream(g));
  TORCH_CHECK(e == hipSuccess, "copy_sdma: hipMemcpyAsync: ", hipGetErrorString(e));
}

// dst (pinned host) <- src (device) on an SDMA engine, ordered on src's current stream through the
// HSA runtime (csrc/bindings/sdma_copy.cpp): the HIP route above still lands on a blit kernel for a
// device -> host copy on this image (profiles/r6_offload_link.md).
void sdma_d2h(Tensor& dst, const Tensor& src, int64_t producer_stream) {
  TORCH_CHECK(dst.is_contiguous() && src.is_contiguous(), "sdma_d2h: contiguous tensors");
  TORCH_CHECK(src.is_cuda() && !dst.is_cuda() && dst.is_pinned(), "sdma_d2h: device source, pinned host destination");
  const int64_t n = dst.numel() * dst.element_size();
  TORCH_CHECK(n == src.numel() * src.element_size(), "sdma_d2h: byte counts differ");
  c10::OptionalDeviceGuard guard(src.device());
  grt::sdma_d2h(dst.data_ptr(), src.data_ptr(), (size_t)n, src.get_device(), cur_stream(src),
                reinterpret_cast<hipStream_t>(producer_stream));
}

py::dict sdma_stats(int64_t device) {
  const grt::SdmaStats st = grt::sdma_stats((int)device);
  py::dict d;
  d["copies"] = st.copies;
  d["bytes"] = st.bytes;
  d["busy_s"] = st.busy_ns * 1e-9;
  d["error"] = st.error;
  d["engine"] = st.engine;
  d["engines_available"] = st.engines_available;
  d["engines_preferred"] = st.engines_preferred;
  return d;
}

// y = x W^T for 1-4 rows (1-16 rows when K % 256 == 0: 3+ rows run on MFMA); swiglu: x = [gate | up]
// [M, 2K] -> y = (silu(gate) * up) W^T
Tensor gemv(const Tensor& x, const Tensor& w, bool swiglu) {
  check_cuda(x, "x");
  check_contig(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == (swiglu ? 2 : 1) * w.size(1),
              swiglu ? "gemv_swiglu: gu [M, 2K], w [N, K]" : "gemv: x [M, K], w [N, K]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "gemv: bf16");
  const int64_t M = x.size(0), N = w.size(0), K = w.size(1);
  TORCH_CHECK((M >= 1 && M <= 4) || (!swiglu && grt::gemv_mfma_ok((int)M, (int)K)),
              "gemv: 1..4 rows (5..16 without swiglu and with K % 256 == 0)");
  TORCH_CHECK(K % 8 == 0 && x.stride(1) == 1 && x.stride(0) % 8 == 0, "gemv: K and row stride multiples of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "gemv: 16-byte alignment");
  TORCH_CHECK(N <= INT32_MAX && K <= INT32_MAX, "gemv: dims");
  c10::OptionalDeviceGuard g(x.device());
  Tensor y = at::empty({M, N}, x.options());
  grt::gemv_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), N, (int)M, (int)N, (int)K, cur_stream(x),
                 swiglu);
  return y;
}

// Decode GEMV with the residual add / RMSNorm folded in (gemv.hip). sumsq: int64 [2, M, 64] fixed-point
// accumulators (zero-initialised once; the producers keep them consistent), slot: 0 / 1.
//   g given: y = bf16(x * rstd * g) W^T with rstd from sumsq[slot] (x = the residual stream h);
//   res given: y = bf16(x W^T) + res, its sums of squares added into sumsq[slot], sumsq[1 - slot]
//   zeroed for the next producer.
//   cos given (qkv, head_dim D = 2 * cos.size(-1), 128 or 64): RoPE in the epilogue at position
//   pos[m]; returns q [M, hq, D], k / v written to cache slot pos[m] of kc / vc (rope_append
//   semantics: bad positions write nothing).
Tensor gemv_fused(const Tensor& x, const Tensor& w, const Tensor& sumsq, int64_t slot, bool swiglu,
                  const c10::optional<Tensor>& g, const c10::optional<Tensor>& res, double eps,
                  const c10::optional<Tensor>& cos, const c10::optional<Tensor>& sin, const c10::optional<Tensor>& pos,
                  const c10::optional<Tensor>& kc, const c10::optional<Tensor>& vc, int64_t hq, int64_t hkv) {
  check_cuda(x, "x");
  check_contig(w, "w");
  check_contig(sumsq, "sumsq");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == (swiglu ? 2 : 1) * w.size(1), "gemv_fused: x [M, K], w [N, K]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "gemv_fused: bf16");
  const int64_t M = x.size(0), N = w.size(0), K = w.size(1);
  TORCH_CHECK(M >= 1 && M <= 4 && K % 8 == 0 && x.stride(1) == 1 && x.stride(0) % 8 == 0, "gemv_fused: 1..4 rows, K % 8");
  TORCH_CHECK(N <= INT32_MAX && K <= INT32_MAX, "gemv_fused: dims");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "gemv_fused: 16-byte alignment");
  TORCH_CHECK(sumsq.scalar_type() == at::kLong && sumsq.numel() % 2 == 0 && sumsq.numel() / 2 >= M * 64 &&
                  (slot == 0 || slot == 1),
              "gemv_fused: sumsq int64 [2, >= M, 64], slot 0 / 1");
  auto* acc = reinterpret_cast<unsigned long long*>(sumsq.data_ptr<int64_t>());
  const int64_t stride = sumsq.numel() / 2;
  grt::GemvFused f{};
  f.x = x.data_ptr(), f.ldx = x.stride(0), f.w = w.data_ptr(), f.M = (int)M, f.N = (int)N, f.K = (int)K;
  f.swiglu = swiglu, f.eps = (float)eps;
  const bool normx = g.has_value() && g->defined();
  const bool resnorm = res.has_value() && res->defined();
  const bool rope = cos.has_value() && cos->defined();
  TORCH_CHECK(!(normx && resnorm) && (normx || resnorm || rope),
              "gemv_fused: g (normalise the input) or res (residual epilogue), and / or cos (RoPE epilogue)");
  TORCH_CHECK(!(rope && (resnorm || swiglu)), "gemv_fused: the RoPE epilogue is for the qkv projection");
  Tensor q;
  if (rope) {
    TORCH_CHECK(sin.has_value() && pos.has_value() && kc.has_value() && vc.has_value(), "gemv_fused: rope needs sin / pos / kc / vc");
    // the head dim is the table's: cos / sin rows hold D / 2 angles
    TORCH_CHECK(cos->dim() >= 1 && (cos->size(-1) == 64 || cos->size(-1) == 32),
                "gemv_fused: rope head_dim (2 * cos.size(-1)) must be 128 or 64");
    const int64_t D = 2 * cos->size(-1);
    check_rope(*cos, *sin, *pos, M, cos->numel() / (D / 2), D);
    TORCH_CHECK(hq > 0 && hkv > 0 && N == (hq + 2 * hkv) * D, "gemv_fused: rope N == (hq + 2 hkv) * head_dim (", D, ")");
    for (const Tensor* c : {&*kc, &*vc}) {
      check_cuda(*c, "cache");
      TORCH_CHECK(c->dim() == 4 && c->size(0) == M && c->size(2) == hkv && c->size(3) == D && c->stride(3) == 1 &&
                      c->scalar_type() == at::kBFloat16,
                  "gemv_fused: cache bf16 [M, L, hkv, head_dim]");
    }
    TORCH_CHECK(vc->sizes() == kc->sizes(), "gemv_fused: kc / vc shapes");
    q = at::empty({M, hq, D}, x.options());
    f.q_out = q.data_ptr(), f.kc = kc->data_ptr(), f.vc = vc->data_ptr();
    f.c_bs = kc->stride(0), f.c_ss = kc->stride(1), f.c_hs = kc->stride(2);
    f.v_bs = vc->stride(0), f.v_ss = vc->stride(1), f.v_hs = vc->stride(2);
    f.cosb = cos->data_ptr<float>(), f.sinb = sin->data_ptr<float>(), f.pos = pos->data_ptr<int32_t>();
    f.rope_S = (int)(cos->numel() / (D / 2)), f.cache_L = (int)kc->size(1), f.hq = (int)hq, f.hkv = (int)hkv;
    f.head_dim = (int)D;
  }
  if (normx) {
    TORCH_CHECK(!swiglu, "gemv_fused: normx and swiglu are exclusive");
    check_contig(*g, "g");
    TORCH_CHECK(g->scalar_type() == at::kBFloat16 && g->numel() == K && reinterpret_cast<uintptr_t>(g->data_ptr()) % 16 == 0,
                "gemv_fused: g bf16 [K], 16-byte aligned");
    f.g = g->data_ptr(), f.sumsq_in = acc + slot * stride;
  } else if (resnorm) {
    check_cuda(*res, "res");
    TORCH_CHECK(res->dim() == 2 && res->size(0) == M && res->size(1) == N && res->stride(1) == 1 &&
                    res->scalar_type() == at::kBFloat16, "gemv_fused: res bf16 [M, N]");
    f.res = res->data_ptr(), f.ldr = res->stride(0);
    f.sumsq_out = acc + slot * stride, f.sumsq_zero = acc + (1 - slot) * stride;
  }
  c10::OptionalDeviceGuard dg(x.device());
  Tensor y = rope ? q : at::empty({M, N}, x.options());
  f.y = rope ? nullptr : y.data_ptr(), f.ldy = N;
  grt::gemv_fused_bf16(f, cur_stream(x));
  return y;
}

// One token per row of logits [B, V] (sample.hip): greedy argmax, or (do_sample) a Gumbel-max draw
// from softmax(logits / temperature) cut to top_k (0: off) and then top_p (1.0: off), with the
// noise of (seed, counter[0], row, index). Returns tokens [B] int64 (next_ids itself when given).
// keep_mask [B, V] uint8: debug output of the kept set. The state tensors (finished, finish_step,
// step, out; with them optionally next_ids, eos_ids, pad_id) add the generate() bookkeeping:
// finished rows emit pad_id, the token goes to next_ids[b] and out[b, step[0]], and a row whose
// winner is one of eos_ids gets finished[b] = true, finish_step[b] = step[0]. max_steps: the caller's
// bound on step[0] + 1 (a step past out's last column writes no column).
Tensor sample_logits(const Tensor& logits, bool do_sample, double temperature, int64_t top_k, double top_p, int64_t seed,
                     const optional<Tensor>& counter, const optional<Tensor>& keep_mask,
                     const optional<Tensor>& finished, const optional<Tensor>& finish_step,
                     const optional<Tensor>& step, const optional<Tensor>& next_ids, const optional<Tensor>& out,
                     const optional<Tensor>& eos_ids, const optional<int64_t>& pad_id, int64_t max_steps,
                     bool candidates) {
  check_cuda(logits, "logits");
  const grt::DType dt = dtype_of(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1, "sample_logits: logits [B, V], B, V >= 1");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V <= INT32_MAX && B <= INT32_MAX, "sample_logits: B, V < 2^31");
  TORCH_CHECK(logits.stride(1) == 1 && (B == 1 || logits.stride(0) >= V),
              "sample_logits: last dimension contiguous, row stride >= V");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % logits.element_size() == 0, "sample_logits: alignment");
  TORCH_CHECK(temperature > 0.0 && std::isfinite(temperature), "sample_logits: temperature must be > 0, got ", temperature);
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "sample_logits: top_p must be in (0, 1], got ", top_p);
  TORCH_CHECK(top_k >= 0, "sample_logits: top_k must be >= 0, got ", top_k);
  auto state_vec = [&](const optional<Tensor>& t, const char* name, int64_t n) -> int64_t* {
    check_contig(*t, name);
    TORCH_CHECK(t->scalar_type() == at::kLong && t->numel() == n && t->device() == logits.device(), "sample_logits: ", name,
                " must be int64 with ", n, " element(s) on the logits' device");
    return t->data_ptr<int64_t>();
  };
  grt::SampleArgs a{};
  a.B = (int)B, a.V = (int)V, a.ld = B == 1 ? V : logits.stride(0);
  a.do_sample = do_sample, a.inv_t = 1.0f / (float)temperature;
  a.top_k = (int)std::min<int64_t>(top_k, V), a.top_p = top_p, a.seed = seed;
  int lg = 0;
  while ((int64_t(1) << lg) < V) ++lg;
  a.mass_scale = std::ldexp(1.0f, std::min(40, 62 - lg));
  if (counter.has_value() && counter->defined()) a.counter = state_vec(counter, "counter", 1);
  if (keep_mask.has_value() && keep_mask->defined()) {
    TORCH_CHECK(do_sample, "sample_logits: keep_mask is an output of the sampling mode");
    check_contig(*keep_mask, "keep_mask");
    TORCH_CHECK(keep_mask->scalar_type() == at::kByte && keep_mask->dim() == 2 && keep_mask->size(0) == B &&
                    keep_mask->size(1) == V && keep_mask->device() == logits.device(),
                "sample_logits: keep_mask uint8 [B, V] on the logits' device");
    a.keep_mask = keep_mask->data_ptr<uint8_t>();
  }
  const bool state = finished.has_value() && finished->defined();
  auto given = [](const optional<Tensor>& t) { return t.has_value() && t->defined(); };
  TORCH_CHECK(state == given(finish_step) && state == given(step) && state == given(out),
              "sample_logits: finished, finish_step, step and out come together");
  TORCH_CHECK(state || (!given(eos_ids) && !pad_id.has_value()), "sample_logits: eos_ids / pad_id need the state tensors");
  TORCH_CHECK(!candidates || !state, "sample_logits: candidates mode takes no state tensors");
  a.candidates = candidates;
  c10::OptionalDeviceGuard dg(logits.device());
  Tensor tokens;
  if (given(next_ids)) {
    state_vec(next_ids, "next_ids", B);
    tokens = *next_ids;
  } else {
    tokens = at::empty({B}, logits.options().dtype(at::kLong));
  }
  a.tokens = tokens.data_ptr<int64_t>();
  if (state) {
    check_contig(*finished, "finished");
    TORCH_CHECK((finished->scalar_type() == at::kBool || finished->scalar_type() == at::kByte) && finished->numel() == B &&
                    finished->device() == logits.device(),
                "sample_logits: finished bool / uint8 [B] on the logits' device");
    a.finished = static_cast<uint8_t*>(finished->data_ptr());
    a.finish_step = state_vec(finish_step, "finish_step", B);
    a.step = state_vec(step, "step", 1);
    check_cuda(*out, "out");
    TORCH_CHECK(out->scalar_type() == at::kLong && out->dim() == 2 && out->size(0) == B && out->size(1) >= 1 &&
                    out->stride(1) == 1 && (B == 1 || out->stride(0) >= out->size(1)) && out->device() == logits.device(),
                "sample_logits: out int64 [B, >= 1], last dimension contiguous, on the logits' device");
    // step[0] lives on the device: the caller states its bound and out must hold that many columns
    TORCH_CHECK(max_steps >= 1 && out->size(1) >= max_steps, "sample_logits: out has ", out->size(1),
                " columns, too narrow for max_steps = ", max_steps);
    a.out = out->data_ptr<int64_t>(), a.out_ld = B == 1 ? out->size(1) : out->stride(0), a.out_cols = out->size(1);
    if (given(eos_ids)) {
      TORCH_CHECK(eos_ids->numel() <= grt::kSampleMaxEos, "sample_logits: at most ", grt::kSampleMaxEos, " EOS ids, got ",
                  eos_ids->numel());
      a.eos = state_vec(eos_ids, "eos_ids", eos_ids->numel()), a.n_eos = (int)eos_ids->numel();
    }
    a.has_pad = pad_id.has_value(), a.pad_id = pad_id.value_or(0);
  }
  grt::sample_logits(logits.data_ptr(), dt, a, cur_stream(logits));
  return tokens;
}

// Accept + draft step of speculative decoding (spec.hip), one sequence, K = drafts.numel() in 1..3.
// Every tensor lives on cand's device and is updated in place; `drafts` holds the drafts the verify
// step was fed and receives the next step's. plan: test hook (the drafts for token n are plan[n ..]).
void spec_advance(const Tensor& cand, const Tensor& drafts, const Tensor& ids, const Tensor& pos, const Tensor& lens,
                  const Tensor& n_step, const Tensor& counter, const Tensor& finished, const Tensor& finish_step,
                  const Tensor& done, const Tensor& out, const Tensor& hist, int64_t prompt_len, int64_t max_new,
                  int64_t max_ngram, int64_t vocab, const optional<Tensor>& plan, const optional<Tensor>& eos_ids) {
  check_cuda(cand, "cand");
  const int64_t K = drafts.numel();
  TORCH_CHECK(K >= 1 && K <= grt::kSpecMaxDrafts, "spec_advance: 1 to ", grt::kSpecMaxDrafts, " drafts, got ", K);
  TORCH_CHECK(max_ngram >= 1 && max_ngram <= INT32_MAX && prompt_len >= 0 && max_new >= 1 && vocab >= 1,
              "spec_advance: max_ngram, max_new, vocab >= 1 and prompt_len >= 0");
  auto vec = [&](const Tensor& t, const char* name, at::ScalarType st, int64_t n, bool exact) {
    check_contig(t, name);
    TORCH_CHECK(t.scalar_type() == st && (exact ? t.numel() == n : t.numel() >= n) && t.device() == cand.device(),
                "spec_advance: ", name, " must hold ", n, " element(s) of its type on cand's device");
    return t.data_ptr();
  };
  grt::SpecAdvanceArgs a{};
  a.cand = (const int64_t*)vec(cand, "cand", at::kLong, K + 1, true);
  a.drafts = (int64_t*)vec(drafts, "drafts", at::kLong, K, true);
  a.ids = (int64_t*)vec(ids, "ids", at::kLong, K + 1, true);
  a.pos = (int32_t*)vec(pos, "pos", at::kInt, K + 1, true);
  a.lens = (int32_t*)vec(lens, "lens", at::kInt, 1, true);
  a.n_step = (int64_t*)vec(n_step, "n_step", at::kLong, 1, true);
  a.counter = (int64_t*)vec(counter, "counter", at::kLong, 1, true);
  TORCH_CHECK(finished.scalar_type() == at::kBool || finished.scalar_type() == at::kByte, "spec_advance: finished bool / uint8");
  a.finished = (uint8_t*)vec(finished, "finished", finished.scalar_type(), 1, true);
  a.finish_step = (int64_t*)vec(finish_step, "finish_step", at::kLong, 1, true);
  TORCH_CHECK(done.scalar_type() == at::kBool || done.scalar_type() == at::kByte, "spec_advance: done bool / uint8");
  a.done = (uint8_t*)vec(done, "done", done.scalar_type(), 1, true);
  a.out = (int64_t*)vec(out, "out", at::kLong, max_new, false);
  a.hist = (int64_t*)vec(hist, "hist", at::kLong, prompt_len + max_new, false);
  a.prompt_len = prompt_len, a.max_new = max_new, a.K = (int)K, a.N = (int)max_ngram, a.vocab = vocab;
  if (plan.has_value() && plan->defined()) {
    a.plan = (const int64_t*)vec(*plan, "plan", at::kLong, 0, false);
    a.plan_len = plan->numel();
  }
  if (eos_ids.has_value() && eos_ids->defined()) {
    TORCH_CHECK(eos_ids->numel() <= grt::kSampleMaxEos, "spec_advance: at most ", grt::kSampleMaxEos, " EOS ids");
    a.eos = (const int64_t*)vec(*eos_ids, "eos_ids", at::kLong, eos_ids->numel(), true);
    a.n_eos = (int)eos_ids->numel();
  }
  c10::OptionalDeviceGuard dg(cand.device());
  grt::spec_advance(a, cur_stream(cand));
}

// y [M, N] = x W^T straight from the NF4 codes of W [N, K] (gemv_nf4.hip; blocksize 64, fp32 absmax),
// 1-4 rows. With h [M, r * targets], lora_b (target i: bf16 [n_i, r]) and lora_off (its first output
// row): rows of target i also get scaling * h[:, i r : (i + 1) r] lora_b[i]^T.
Tensor nf4_gemv(const Tensor& x, const Tensor& q, const Tensor& absmax, int64_t N, int64_t K,
                const optional<Tensor>& h, const optional<std::vector<Tensor>>& lora_b,
                const optional<std::vector<int64_t>>& lora_off, double scaling) {
  check_cuda(x, "x");
  check_contig(q, "qweight");
  check_contig(absmax, "absmax");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == K, "nf4_gemv: x [M, K]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "nf4_gemv: x bf16");
  TORCH_CHECK(q.is_cuda() && absmax.is_cuda() && q.scalar_type() == at::kByte && absmax.scalar_type() == at::kFloat,
              "nf4_gemv: qweight uint8, absmax fp32, on the GPU");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= 4, "nf4_gemv: 1..4 rows");
  TORCH_CHECK(N >= 1 && K >= 64 && K % 64 == 0 && N <= INT32_MAX && K <= (1 << 30), "nf4_gemv: K % 64 == 0");
  TORCH_CHECK(q.numel() * 2 == N * K && absmax.numel() * 64 == N * K, "nf4_gemv: nf4 shapes (blocksize 64)");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) >= K && x.stride(0) % 8 == 0, "nf4_gemv: x row stride >= K, multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "nf4_gemv: 16-byte alignment");
  grt::Nf4Gemv f{};
  f.x = x.data_ptr(), f.ldx = x.stride(0), f.q = q.data_ptr<uint8_t>(), f.absmax = absmax.data_ptr<float>();
  f.M = (int)M, f.N = (int)N, f.K = (int)K;
  const bool lora = h.has_value() || lora_b.has_value() || lora_off.has_value();
  if (lora) {
    TORCH_CHECK(h.has_value() && lora_b.has_value() && lora_off.has_value(), "nf4_gemv: h, lora_b and lora_off go together");
    const int64_t T = (int64_t)lora_b->size();
    TORCH_CHECK(T >= 1 && T <= grt::kNf4GemvMaxTargets && (int64_t)lora_off->size() == T, "nf4_gemv: 1..4 targets");
    const int64_t r = (*lora_b)[0].dim() == 2 ? (*lora_b)[0].size(1) : 0;
    TORCH_CHECK(r >= 8 && r <= 64 && r % 8 == 0, "nf4_gemv: r <= 64, r % 8 == 0");
    TORCH_CHECK(h->is_cuda() && h->dim() == 2 && h->scalar_type() == at::kBFloat16 && h->size(0) == M &&
                    h->size(1) == r * T && h->stride(1) == 1, "nf4_gemv: h bf16 [M, r * targets]");
    for (int64_t i = 0; i < T; ++i) {
      const Tensor& b = (*lora_b)[i];
      const int64_t off = (*lora_off)[i];
      TORCH_CHECK(b.is_cuda() && b.dim() == 2 && b.scalar_type() == at::kBFloat16 && b.is_contiguous() && b.size(1) == r &&
                      b.size(0) >= 1, "nf4_gemv: lora_b bf16 [n_i, r] contiguous");
      TORCH_CHECK(off >= 0 && off % 4 == 0 && off + b.size(0) <= N, "nf4_gemv: lora_off % 4 == 0, target inside [0, N)");
      for (int64_t j = 0; j < i; ++j)
        TORCH_CHECK(off + b.size(0) <= f.off[j] || f.off[j] + f.n[j] <= off, "nf4_gemv: targets overlap");
      f.b[i] = b.data_ptr(), f.off[i] = (int)off, f.n[i] = (int)b.size(0);
    }
    f.h = h->data_ptr(), f.ldh = h->stride(0), f.r = (int)r, f.targets = (int)T, f.scaling = (float)scaling;
  }
  c10::OptionalDeviceGuard g(x.device());
  Tensor y = at::empty({M, N}, x.options());
  f.y = y.data_ptr();
  grt::gemv_nf4(f, cur_stream(x));
  return y;
}

// ------------------------------------------------------------------ embedding
Tensor embedding_fwd(const Tensor& ids, const Tensor& w) {
  check_contig(ids, "ids");
  check_contig(w, "weight");
  TORCH_CHECK(ids.scalar_type() == at::kLong && w.dim() == 2, "embedding: int64 ids, 2-D weight");
  const int64_t d = w.size(1);
  TORCH_CHECK(d % 8 == 0, "embedding: row width must be a multiple of 8");
  c10::OptionalDeviceGuard g(w.device());
  auto out = at::empty({ids.numel(), d}, w.options());
  if (ids.numel() == 0) return out;
  grt::embedding_fwd(dtype_of(w), ids.data_ptr<int64_t>(), w.data_ptr(), out.data_ptr(), ids.numel(), (int)d,
                     w.size(0), cur_stream(w));
  return out;
}

void embedding_bwd(const Tensor& dy, const Tensor& ids, const Tensor& dw, bool accumulate) {
  check_contig(dy, "dy");
  check_contig(dw, "dw");
  check_contig(ids, "ids");
  TORCH_CHECK(ids.scalar_type() == at::kLong, "embedding_bwd: int64 ids");
  TORCH_CHECK(dy.dim() == 2 && dw.dim() == 2 && dy.size(1) == dw.size(1) && dy.size(0) == ids.numel(),
              "embedding_bwd: shapes");
  TORCH_CHECK(dy.size(1) % 8 == 0, "embedding_bwd: row width must be a multiple of 8");
  TORCH_CHECK(dy.scalar_type() == dw.scalar_type(), "embedding_bwd: dtype");
  TORCH_CHECK(ids.device() == dy.device() && dw.device() == dy.device(), "embedding_bwd: ids, dy and dw on one device");
  c10::OptionalDeviceGuard g(dy.device());
  const int64_t V = dw.size(0);
  if (ids.numel() == 0) {  // no token: every row is unhit
    if (!accumulate) dw.zero_();
    return;
  }
  auto flat = ids.reshape({-1});
  auto sorted = flat.sort();
  auto vals = std::get<0>(sorted);
  auto order = std::get<1>(sorted).contiguous();
  // segment bounds of every vocabulary row by binary search: no unique() (its output size would
  // force a device->host sync in the middle of the backward)
  auto rows = at::arange(V, vals.options());
  auto row_start = at::searchsorted(vals, rows, /*out_int32=*/true, /*right=*/false);
  auto row_end = at::searchsorted(vals, rows, /*out_int32=*/true, /*right=*/true);
  grt::embedding_bwd(dtype_of(dy), dy.data_ptr(), order.data_ptr<int64_t>(), row_start.data_ptr<int32_t>(),
                     row_end.data_ptr<int32_t>(), dw.data_ptr(), V, (int)dy.size(1), accumulate, cur_stream(dy));
}

// ------------------------------------------------------------------ weight-gradient GEMM
// out[P][Q] (+)= x[R][P]^T @ y[R][Q]  (dW = dY^T X); returns false when the shape is unsupported
bool gemm_wgrad(const Tensor& x, const Tensor& y, const Tensor& out, bool accumulate, int64_t mode) {
  TORCH_CHECK(x.dim() == 2 && y.dim() == 2 && out.dim() == 2, "gemm_wgrad: 2-D operands");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16 &&
                  out.scalar_type() == at::kBFloat16, "gemm_wgrad: bf16 operands");
  TORCH_CHECK(x.is_cuda() && y.is_cuda() && out.is_cuda(), "gemm_wgrad: device tensors");
  const int64_t R = x.size(0), P = x.size(1), Q = y.size(1);
  TORCH_CHECK(y.size(0) == R && out.size(0) == P && out.size(1) == Q, "gemm_wgrad: shape mismatch");
  if (x.stride(1) != 1 || y.stride(1) != 1 || out.stride(1) != 1) return false;
  if (x.stride(0) % 8 || y.stride(0) % 8 || out.stride(0) % 8) return false;
  for (const Tensor* t : std::initializer_list<const Tensor*>{&x, &y, &out})
    if (reinterpret_cast<uintptr_t>(t->data_ptr()) % 16) return false;
  if (P > INT32_MAX || Q > INT32_MAX || R > INT32_MAX || !grt::gemm_tt_supported((int)P, (int)Q, (int)R))
    return false;
  c10::OptionalDeviceGuard g(x.device());
  grt::GemmTTParams p{x.data_ptr(), y.data_ptr(), out.data_ptr(), (int)P, (int)Q, (int)R,
                      x.stride(0), y.stride(0), out.stride(0), accumulate ? 1 : 0};
  grt::gemm_tt(p, cur_stream(x), (int)mode);
  return true;
}

// ------------------------------------------------------------------ projection GEMM
// out[M][N] (+)= a[M][K] @ b[N][K]^T on the hand-written MFMA kernel; returns false (nothing
// launched) when the shape / layout is outside what the kernel tiles, so callers can fall back.
bool gemm_supported(const Tensor& a, const Tensor& b, const Tensor& out) {
  if (a.dim() != 2 || b.dim() != 2 || out.dim() != 2) return false;
  if (a.scalar_type() != at::kBFloat16 || b.scalar_type() != at::kBFloat16 || out.scalar_type() != at::kBFloat16)
    return false;
  if (!a.is_cuda() || !b.is_cuda() || !out.is_cuda()) return false;
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  if (b.size(1) != K || out.size(0) != M || out.size(1) != N) return false;
  if (a.stride(1) != 1 || b.stride(1) != 1 || out.stride(1) != 1) return false;
  if (a.stride(0) % 8 || b.stride(0) % 8 || out.stride(0) % 8) return false;
  for (const Tensor* t : std::initializer_list<const Tensor*>{&a, &b, &out})
    if (reinterpret_cast<uintptr_t>(t->data_ptr()) % 16) return false;
  // the kernel's buffer descriptors address A and B with 32-bit byte offsets
  if (M * a.stride(0) * 2 >= (int64_t(1) << 31) || N * b.stride(0) * 2 >= (int64_t(1) << 31)) return false;
  return grt::gemm_nt_supported(M, N, K);
}

bool gemm_nt(const Tensor& a, const Tensor& b, const Tensor& out, bool accumulate, int64_t variant) {
  if (!gemm_supported(a, b, out)) return false;
  c10::OptionalDeviceGuard g(a.device());
  grt::GemmParams p{a.data_ptr(), b.data_ptr(), out.data_ptr(), (int)a.size(0), (int)b.size(0), (int)a.size(1),
                    a.stride(0), b.stride(0), out.stride(0), accumulate ? 1 : 0, grt::GEMM_EPI_STORE, (int)variant};
  grt::gemm_nt(p, cur_stream(a));
  return true;
}

// out[P][Q] (+)= x[R][P]^T @ y[R][Q] (dW = dY^T X) on the half-tile MFMA kernel reading the
// token-major operands through transposed LDS reads; false when the shape does not tile
bool gemm_wgrad2(const Tensor& x, const Tensor& y, const Tensor& out, bool accumulate) {
  if (x.dim() != 2 || y.dim() != 2 || out.dim() != 2) return false;
  if (x.scalar_type() != at::kBFloat16 || y.scalar_type() != at::kBFloat16 || out.scalar_type() != at::kBFloat16)
    return false;
  if (!x.is_cuda() || !y.is_cuda() || !out.is_cuda()) return false;
  const int64_t R = x.size(0), P = x.size(1), Q = y.size(1);
  if (y.size(0) != R || out.size(0) != P || out.size(1) != Q) return false;
  if (x.stride(1) != 1 || y.stride(1) != 1 || out.stride(1) != 1) return false;
  if (x.stride(0) % 8 || y.stride(0) % 8 || out.stride(0) % 8) return false;
  for (const Tensor* t : std::initializer_list<const Tensor*>{&x, &y, &out})
    if (reinterpret_cast<uintptr_t>(t->data_ptr()) % 16) return false;
  if (P % 256 || Q % 256 || R % 64 || R == 0 || P > INT32_MAX || Q > INT32_MAX || R > INT32_MAX) return false;
  c10::OptionalDeviceGuard g(x.device());
  grt::GemmParams p{x.data_ptr(), y.data_ptr(), out.data_ptr(), (int)P, (int)Q, (int)R,
                    x.stride(0), y.stride(0), out.stride(0), accumulate ? 1 : 0, grt::GEMM_EPI_STORE, 0};
  grt::gemm_tt2(p, cur_stream(x));
  return true;
}

// out[M][N] (+)= a[M][K] @ b[K][N] (dX = dY W on W as stored [N_out][K_in]); false when unsupported
bool gemm_nn(const Tensor& a, const Tensor& b, const Tensor& out, bool accumulate) {
  if (a.dim() != 2 || b.dim() != 2 || out.dim() != 2) return false;
  if (a.scalar_type() != at::kBFloat16 || b.scalar_type() != at::kBFloat16 || out.scalar_type() != at::kBFloat16)
    return false;
  if (!a.is_cuda() || !b.is_cuda() || !out.is_cuda()) return false;
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  if (b.size(0) != K || out.size(0) != M || out.size(1) != N) return false;
  if (a.stride(1) != 1 || b.stride(1) != 1 || out.stride(1) != 1) return false;
  if (a.stride(0) % 8 || b.stride(0) % 8 || out.stride(0) % 8) return false;
  for (const Tensor* t : std::initializer_list<const Tensor*>{&a, &b, &out})
    if (reinterpret_cast<uintptr_t>(t->data_ptr()) % 16) return false;
  if (M % 256 || N % 256 || K % 64 || K == 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return false;
  c10::OptionalDeviceGuard g(a.device());
  grt::GemmParams p{a.data_ptr(), b.data_ptr(), out.data_ptr(), (int)M, (int)N, (int)K,
                    a.stride(0), b.stride(0), out.stride(0), accumulate ? 1 : 0, grt::GEMM_EPI_STORE, 0};
  grt::gemm_nn(p, cur_stream(a));
  return true;
}

// ------------------------------------------------------------------ xGMI IPC collectives
int64_t ipc_alloc(int64_t nbytes, bool fine_grained, int64_t device) {
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  return reinterpret_cast<int64_t>(grt::ipc_malloc(nbytes, fine_grained));
}
void ipc_free_ptr(int64_t p, int64_t device) {
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  grt::ipc_free(reinterpret_cast<void*>(p));
}
py::bytes ipc_handle(int64_t p, int64_t device) {
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  char h[grt::kIpcHandleBytes];
  grt::ipc_get_handle(reinterpret_cast<void*>(p), h);
  return py::bytes(h, grt::kIpcHandleBytes);
}
int64_t ipc_open(const py::bytes& handle, int64_t device) {
  std::string h = handle;
  TORCH_CHECK((int)h.size() == grt::kIpcHandleBytes, "ipc_open: handle must be ", grt::kIpcHandleBytes, " bytes");
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  return reinterpret_cast<int64_t>(grt::ipc_open_handle(h.data()));
}
void ipc_close(int64_t p, int64_t device) {
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  grt::ipc_close_handle(reinterpret_cast<void*>(p));
}

grt::IpcPeers make_peers(const std::vector<int64_t>& staging, const std::vector<int64_t>& result,
                         const std::vector<int64_t>& signal, const Tensor& err, int64_t cap, int64_t rank,
                         int64_t timeout_ticks) {
  const int64_t W = (int64_t)staging.size();
  TORCH_CHECK(W >= 1 && W <= grt::kIpcMaxRanks, "ipc: world size must be 1..", grt::kIpcMaxRanks);
  TORCH_CHECK((int64_t)result.size() == W && (int64_t)signal.size() == W, "ipc: pointer lists differ in length");
  TORCH_CHECK(rank >= 0 && rank < W, "ipc: bad rank");
  check_contig(err, "err");
  TORCH_CHECK(err.scalar_type() == at::kInt && err.numel() >= 1, "ipc: err must be an int32 device tensor");
  grt::IpcPeers p{};
  for (int64_t i = 0; i < W; ++i) {
    TORCH_CHECK(staging[i] && result[i] && signal[i], "ipc: null peer buffer");
    p.staging[i] = reinterpret_cast<void*>(staging[i]);
    p.result[i] = reinterpret_cast<void*>(result[i]);
    p.signal[i] = reinterpret_cast<uint32_t*>(signal[i]);
  }
  p.err = reinterpret_cast<uint32_t*>(err.data_ptr());
  p.cap = cap;
  p.rank = (int)rank;
  p.world = (int)W;
  p.timeout_ticks = (uint64_t)timeout_ticks;
  return p;
}

void ipc_allreduce(const std::vector<int64_t>& staging, const std::vector<int64_t>& result,
                   const std::vector<int64_t>& signal, const Tensor& err, int64_t cap, int64_t rank, int64_t epoch,
                   int64_t timeout_ticks, const Tensor& in, const Tensor& out, bool two_shot, double scale) {
  const grt::IpcPeers p = make_peers(staging, result, signal, err, cap, rank, timeout_ticks);
  check_contig(in, "in");
  check_contig(out, "out");
  TORCH_CHECK(in.device() == err.device() && out.device() == err.device(), "ipc: tensors on another device");
  TORCH_CHECK(in.scalar_type() == out.scalar_type() && in.numel() == out.numel(), "ipc: in/out mismatch");
  const int64_t nbytes = in.numel() * in.element_size();
  TORCH_CHECK(nbytes % 16 == 0, "ipc: message must be a multiple of 16 bytes (pad it)");
  TORCH_CHECK(nbytes <= cap, "ipc: message of ", nbytes, " bytes exceeds the buffer (", cap, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(in.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "ipc: 16-byte alignment required");
  c10::OptionalDeviceGuard g(in.device());
  grt::ipc_allreduce(p, (uint32_t)epoch, dtype_of(in), in.data_ptr(), out.data_ptr(), nbytes, two_shot, (float)scale,
                     cur_stream(in));
}

void ipc_barrier(const std::vector<int64_t>& staging, const std::vector<int64_t>& result,
                 const std::vector<int64_t>& signal, const Tensor& err, int64_t cap, int64_t rank, int64_t epoch,
                 int64_t timeout_ticks) {
  const grt::IpcPeers p = make_peers(staging, result, signal, err, cap, rank, timeout_ticks);
  c10::OptionalDeviceGuard g(err.device());
  grt::ipc_barrier(p, (uint32_t)epoch, cur_stream(err));
}

// A HIP stream whose dispatches may only use the CUs set in `mask` (32 CUs per word). Used for
// side-stream work (the overlapped optimizer) that must leave the other CUs to the compute
// stream's GEMMs instead of filling every CU's wave slots. Returned as an integer handle for
// torch.cuda.ExternalStream; it lives for the process (streams are few and reused).
int64_t cu_masked_stream(const std::vector<int64_t>& mask, int64_t device) {
  TORCH_CHECK(!mask.empty(), "cu_masked_stream: empty mask");
  std::vector<uint32_t> words(mask.size());
  bool any = false;
  for (size_t i = 0; i < mask.size(); ++i) {
    TORCH_CHECK(mask[i] >= 0 && mask[i] <= 0xffffffffLL, "cu_masked_stream: mask word out of range");
    words[i] = (uint32_t)mask[i];
    any = any || words[i] != 0;
  }
  TORCH_CHECK(any, "cu_masked_stream: mask selects no CU");
  c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  hipStream_t s = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)words.size(), words.data());
  TORCH_CHECK(e == hipSuccess, "hipExtStreamCreateWithCUMask: ", hipGetErrorString(e));
  return reinterpret_cast<int64_t>(s);
}

std::vector<int64_t> stream_cu_mask(int64_t stream, int64_t words) {
  TORCH_CHECK(words > 0 && words <= 64, "stream_cu_mask: 1..64 words");
  std::vector<uint32_t> w((size_t)words, 0u);
  const hipError_t e = hipExtStreamGetCUMask(reinterpret_cast<hipStream_t>(stream), (uint32_t)words, w.data());
  TORCH_CHECK(e == hipSuccess, "hipExtStreamGetCUMask: ", hipGetErrorString(e));
  return std::vector<int64_t>(w.begin(), w.end());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gke_ray_train_amd HIP kernels for gfx950 (MI355X)";
  m.def("rmsnorm_fwd", &rmsnorm_fwd, py::arg("x"), py::arg("residual"), py::arg("w"), py::arg("eps"),
        py::arg("pad") = 0);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("h"), py::arg("w"), py::arg("rstd"), py::arg("dres"),
        py::arg("dw_out") = py::none(), py::arg("accumulate") = false);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("swiglu_fwd", &swiglu_fwd, py::arg("gu"), py::arg("pad") = 0);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("rope_bwd", &rope_bwd);
  m.def("rope_append", &rope_append);
  m.def("rope_append_fp8", &rope_append_fp8, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("pos"), py::arg("hq"),
        py::arg("hkv"), py::arg("D"), py::arg("S"), py::arg("kc"), py::arg("vc"), py::arg("k_scale"), py::arg("v_scale"),
        py::arg("tpr"), py::arg("k_out") = py::none());
  m.def("kv_fp8_dequant", &kv_fp8_dequant);
  m.def("scale_add_pe", &scale_add_pe);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_bwd", &dropout_bwd);
  m.def("dropout_fwd_seeded", &dropout_fwd_seeded);
  m.def("lora_down", &lora_down, py::arg("x"), py::arg("a"), py::arg("p"), py::arg("seed"), py::arg("offset"),
        py::arg("want_xd"), py::arg("h_out") = py::none(), py::arg("hscale") = 1.0);
  m.def("lora_dx", &lora_dx, py::arg("g"), py::arg("at"), py::arg("dx"), py::arg("p"), py::arg("seed"),
        py::arg("offset"), py::arg("accumulate"), py::arg("dx_in") = py::none(), py::arg("gscale") = 1.0);
  m.def("lora_refresh", &lora_refresh, py::arg("bs"), py::arg("offs"), py::arg("w"), py::arg("wt"), py::arg("col0"),
        py::arg("wt_row0") = -1);
  m.def("lora_g", &lora_g, py::arg("a"), py::arg("bt"), py::arg("c"), py::arg("alpha"), py::arg("accumulate"));
  m.def("lora_g_group", &lora_g_group, py::arg("a"), py::arg("bt"), py::arg("c"), py::arg("alpha"),
        py::arg("accumulate"));
  m.def("lora_tred", &lora_tred, py::arg("a"), py::arg("h"), py::arg("out"), py::arg("alpha"), py::arg("accumulate"),
        py::arg("transpose"));
  m.def("lora_tred_group", &lora_tred_group, py::arg("a"), py::arg("h"), py::arg("out"), py::arg("alpha"),
        py::arg("accumulate"));
  m.def("dropout_bwd_seeded", &dropout_bwd_seeded);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("sumsq_blocks", &sumsq_blocks);
  m.def("lds_fill", [](int64_t pattern, int64_t device) {
    c10::OptionalDeviceGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
    grt::lds_fill((uint32_t)pattern, c10::hip::getCurrentHIPStream((c10::DeviceIndex)device).stream());
  }, "test support: fill every CU's LDS with a 32-bit pattern (stale-LDS-read detection)");
  m.def("sumsq", &sumsq);
  m.def("clip_finalize", &clip_finalize);
  m.def("adamw", &adamw, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("master"),
        py::arg("hyper"), py::arg("gscale"), py::arg("max_blocks") = 0, py::arg("index_offset") = 0);
  m.def("adamw_t", &adamw_t);
  m.def("adamw8", &adamw8, py::arg("p"), py::arg("g"), py::arg("codes_m"), py::arg("absmax_m"), py::arg("codes_v"),
        py::arg("absmax_v"), py::arg("master"), py::arg("hyper"), py::arg("gscale"), py::arg("max_blocks") = 0,
        py::arg("index_offset") = 0);
  m.def("quantize_blockwise8", &quantize_blockwise8, py::arg("x"), py::arg("codes"), py::arg("absmax"),
        py::arg("signed"));
  m.def("dequantize_blockwise8", &dequantize_blockwise8, py::arg("codes"), py::arg("absmax"), py::arg("out"),
        py::arg("signed"));
  m.def("scale_", &scale_);
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("scale"),
        py::arg("causal"), py::arg("seqlens_k"), py::arg("dropout_p") = 0.0, py::arg("seed") = 0,
        py::arg("cu_seqlens") = py::none(), py::arg("max_seqlen") = 0, py::arg("o_t") = py::none());
  m.def("attn_bwd", &attn_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("scale"), py::arg("causal"),
        py::arg("seqlens_k"), py::arg("dropout_p") = 0.0, py::arg("seed") = 0, py::arg("rope_cos") = py::none(),
        py::arg("rope_sin") = py::none(), py::arg("cu_seqlens") = py::none(), py::arg("max_seqlen") = 0,
        py::arg("dqkv_t") = py::none());
  m.def("rope_attn_fwd_d64", &rope_attn_fwd_d64, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("o"),
        py::arg("B"), py::arg("S"), py::arg("hq"), py::arg("hkv"), py::arg("scale"), py::arg("causal"),
        py::arg("cu_seqlens") = py::none(), py::arg("max_seqlen") = 0,
        "bf16 head_dim 64: RoPE + flash attention straight from the fused QKV rows (packed with cu_seqlens) -> lse");
  m.def("rope_attn_bwd_d64", &rope_attn_bwd_d64, py::arg("do"), py::arg("qkv"), py::arg("cos"), py::arg("sin"),
        py::arg("o"), py::arg("lse"), py::arg("dqkv"), py::arg("B"), py::arg("S"), py::arg("hq"), py::arg("hkv"),
        py::arg("scale"), py::arg("causal"), py::arg("cu_seqlens") = py::none(), py::arg("max_seqlen") = 0,
        "backward of rope_attn_fwd_d64: un-rotated dQ / dK and dV into the columns of dqkv (every element written)");
  m.def("attn_set_schedule", &grt::attn_set_schedule,
        "bf16 attention causal-pair / XCD-grouped schedule, bit mask: 1 = forward, 2 = dQ, 4 = dK/dV");
  m.def("attn_get_schedule", &grt::attn_get_schedule);
  m.def("attn_set_dkdv_form", &grt::attn_set_dkdv_form, "dK / dV kernel: 1 = 4-wave, 2 = wave-pair (default)");
  m.def("attn_get_dkdv_form", &grt::attn_get_dkdv_form);
  m.def("attn_set_dma_fast", &grt::attn_set_dma_fast, "1 = hoisted LDS-DMA addressing (default), 0 = clamped per tile");
  m.def("ew_set_fast", &grt::ew_set_fast, "1 = single-pass RoPE (D = 128) / SwiGLU kernels (default), 0 = grid-stride kernels");
  m.def("attn_set_skip_dead", &grt::attn_set_skip_dead,
        "1 = forward / dK-dV waves skip the causal tiles they mask entirely (default), 0 = compute them");
  m.def("nf4_quantize", &nf4_quantize);
  m.def("nf4_dequantize", &nf4_dequantize);
  m.def("nf4_dequantize_t", &nf4_dequantize_t);
  m.def("nf4_dequantize_into", &nf4_dequantize_into);
  m.def("rmsnorm_bwd_dx", &rmsnorm_bwd_dx);
  m.def("swiglu_fwd_t", &swiglu_fwd_t);
  m.def("swiglu_bwd_t", &swiglu_bwd_t);
  m.def("transpose_into", &transpose_into);
  m.def("copy_sdma", &copy_sdma);
  m.def("sdma_d2h", &sdma_d2h, py::arg("dst"), py::arg("src"), py::arg("producer_stream") = 0,
        "pinned host <- device on an SDMA engine, ordered on the source's current stream; producer_stream "
        "(a raw stream handle): the stream whose work so far wrote src");
  m.def("sdma_stats", &sdma_stats, "copies / bytes / worker busy seconds / first error of the SDMA copier");
  m.def("sdma_clear_error", [](int64_t device) { grt::sdma_clear_error((int)device); });
  m.def("gemv", &gemv, py::arg("x"), py::arg("w"), py::arg("swiglu") = false);
  m.def("gemv_fused", &gemv_fused, py::arg("x"), py::arg("w"), py::arg("sumsq"), py::arg("slot"),
        py::arg("swiglu") = false, py::arg("g") = py::none(), py::arg("res") = py::none(), py::arg("eps") = 1e-5,
        py::arg("cos") = py::none(), py::arg("sin") = py::none(), py::arg("pos") = py::none(),
        py::arg("kc") = py::none(), py::arg("vc") = py::none(), py::arg("hq") = 0, py::arg("hkv") = 0);
  m.def("nf4_gemv", &nf4_gemv, py::arg("x"), py::arg("qweight"), py::arg("absmax"), py::arg("N"), py::arg("K"),
        py::arg("h") = py::none(), py::arg("lora_b") = py::none(), py::arg("lora_off") = py::none(),
        py::arg("scaling") = 1.0);
  m.def("sample_logits", &sample_logits, py::arg("logits"), py::arg("do_sample") = false, py::arg("temperature") = 1.0,
        py::arg("top_k") = 0, py::arg("top_p") = 1.0, py::arg("seed") = 0, py::arg("counter") = py::none(),
        py::arg("keep_mask") = py::none(), py::arg("finished") = py::none(), py::arg("finish_step") = py::none(),
        py::arg("step") = py::none(), py::arg("next_ids") = py::none(), py::arg("out") = py::none(),
        py::arg("eos_ids") = py::none(), py::arg("pad_id") = py::none(), py::arg("max_steps") = 1,
        py::arg("candidates") = false);
  m.def("spec_advance", &spec_advance, py::arg("cand"), py::arg("drafts"), py::arg("ids"), py::arg("pos"),
        py::arg("lens"), py::arg("n_step"), py::arg("counter"), py::arg("finished"), py::arg("finish_step"),
        py::arg("done"), py::arg("out"), py::arg("hist"), py::arg("prompt_len"), py::arg("max_new"),
        py::arg("max_ngram"), py::arg("vocab"), py::arg("plan") = py::none(), py::arg("eos_ids") = py::none());
  m.def("attn_decode_multi", &attn_decode_multi);
  m.def("attn_decode_multi_d64", &attn_decode_multi_d64);
  m.def("attn_decode", &attn_decode);
  m.def("attn_decode_d64", &attn_decode_d64);
  m.def("attn_decode_fp8", &attn_decode_fp8);
  m.def("attn_decode_fp8_d64", &attn_decode_fp8_d64);
  m.def("attn_decode_d64_partials", &attn_decode_d64_partials,
        "test support: attn_decode_d64 and its per-split (o, max, sum) partial states");
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("gemm_wgrad", &gemm_wgrad, py::arg("x"), py::arg("y"), py::arg("out"), py::arg("accumulate"),
        py::arg("mode") = 0);
  m.def("gemm_supported", &gemm_supported, py::arg("a"), py::arg("b"), py::arg("out"));
  m.def("gemm_nt", &gemm_nt, py::arg("a"), py::arg("b"), py::arg("out"), py::arg("accumulate") = false,
        py::arg("variant") = 0);
  m.def("gemm_wgrad2", &gemm_wgrad2, py::arg("x"), py::arg("y"), py::arg("out"), py::arg("accumulate") = false);
  m.def("gemm_nn", &gemm_nn, py::arg("a"), py::arg("b"), py::arg("out"), py::arg("accumulate") = false);
  m.def("ipc_alloc", &ipc_alloc);
  m.def("ipc_free", &ipc_free_ptr);
  m.def("ipc_handle", &ipc_handle);
  m.def("ipc_open", &ipc_open);
  m.def("ipc_close", &ipc_close);
  m.def("ipc_allreduce", &ipc_allreduce);
  m.def("ipc_barrier", &ipc_barrier);
  m.def("cu_masked_stream", &cu_masked_stream);
  m.def("stream_cu_mask", &stream_cu_mask);
  m.attr("IPC_MAX_RANKS") = grt::kIpcMaxRanks;
  m.attr("IPC_SIGNAL_BYTES") = grt::kIpcSignalBytes;
}
