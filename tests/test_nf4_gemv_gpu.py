"""Decode GEMV from NF4 codes with the LoRA epilogue (csrc/kernels/gemv_nf4.hip): the binding against
float64 on the exact NF4 weight, its guards, bitwise stability, ``NF4Linear`` / ``LoraLinear`` routing
and graph / eager generation from a 4-bit base.

Bounds (derived, not measured): the output is one bf16 rounding of an fp32 sum, so
|y - y64| <= 2^-7 |y64| + (terms + 64) 2^-24 sum|x_k w_k| covers the rounding (unit roundoff 2^-8,
doubled) and a worst-case fp32 accumulation in any order with slack for the per-block factoring of
absmax. The reference weight is fp32 level * fp32 absmax (``_ref.nf4_dequantize(..., float32)``), not
the bf16-rounded weight of the dequantisers."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child process starts from this file, not from pytest
    sys.path.insert(0, ROOT)

DEV = "cuda"
QNAN = 0x7FC00000
SCALING = 1.75


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _weights(N, K, g):
    """Random weights, every 64-block scaled by 2^U(-6, 6) (a wrong block index shows), quantised by
    the GPU quantiser -> (codes, absmax, W32 [N, K] the exact NF4 value)."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    w = torch.randn(N * K // 64, 64, device=DEV, generator=g)
    w = w * torch.exp2(torch.rand(N * K // 64, 1, device=DEV, generator=g) * 12 - 6)
    q, a = ops.nf4_quantize(w.view(-1), 64)
    return q, a, _ref.nf4_dequantize(q, a, N * K, 64, torch.float32).view(N, K)


def _x(M, K, g, strided):
    """bf16 rows, each different; ``strided``: a view of a wider buffer whose other columns are NaN."""
    vals = (torch.randn(M, K, device=DEV, generator=g) * torch.arange(1, M + 1, device=DEV)[:, None]).bfloat16()
    if not strided:
        return vals
    buf = torch.full((M, K + 64), float("nan"), device=DEV, dtype=torch.bfloat16)
    buf[:, :K] = vals
    return buf[:, :K]


def _check(y, y64, mag, terms, what, extra=None):
    tol = 2.0 ** -7 * y64.abs() + (terms + 64) * 2.0 ** -24 * mag
    if extra is not None:
        tol = tol + extra
    err = (y.double() - y64).abs()
    assert torch.isfinite(y.float()).all(), f"{what}: non-finite output"
    ratio = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert bool((err <= tol).all()), f"{what}: worst error / bound = {ratio:.3g}"


# ------------------------------------------------------------------ 1. kernel against float64
@pytest.mark.parametrize("M,N,K,strided", [
    (1, 4, 64, False),       # one block per row, nearly every lane idle
    (3, 20, 192, True),      # partial last workgroup, blocks not divisible among waves
    (4, 20, 2112, False),    # K-loop tail
    (2, 768, 256, True),     # regular mid-size case
    (1, 64, 8192, False),    # a full Llama-size row (K split over 4 waves)
    (2, 12, 4160, True),     # the 2-wave K split, with a tail
])
def test_kernel_matches_float64(M, N, K, strided):
    g = _gen(1000 * M + N + K)
    q, a, w32 = _weights(N, K, g)
    x = _x(M, K, g, strided)
    y = _C().nf4_gemv(x, q, a, N, K)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    _check(y, y64, mag, K, f"nf4_gemv {M}x{N}x{K}")


# ------------------------------------------------------------------ 2. LoRA epilogue
def _lora_case(M, N, K, r, spans, g):
    q, a, w32 = _weights(N, K, g)
    x = _x(M, K, g, False)
    h = torch.randn(M, r * len(spans), device=DEV, generator=g).bfloat16()
    Bs = [(torch.randn(n, r, device=DEV, generator=g) * 0.05).bfloat16() for _, n in spans]
    offs = [off for off, _ in spans]
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    lmag = torch.zeros_like(mag)
    for i, ((off, n), b) in enumerate(zip(spans, Bs)):
        hi = h[:, i * r:(i + 1) * r].double()
        y64[:, off:off + n] += SCALING * (hi @ b.double().t())
        lmag[:, off:off + n] += abs(SCALING) * (hi.abs() @ b.double().abs().t())
    return x, q, a, h, Bs, offs, y64, mag, lmag


@pytest.mark.parametrize("M,N,K,r,spans", [
    (2, 768, 256, 64, [(0, 512), (512, 128), (640, 128)]),   # three targets covering every row
    (3, 768, 256, 16, [(0, 256), (512, 256)]),               # the middle 256 rows bare
    (1, 20, 192, 8, [(0, 20)]),                              # one target, partial last workgroup
    (4, 64, 8192, 8, [(4, 30)]),                             # target ends off a 4-row group, K split
])
def test_lora_epilogue_matches_float64(M, N, K, r, spans):
    g = _gen(7 * N + K + r)
    x, q, a, h, Bs, offs, y64, mag, lmag = _lora_case(M, N, K, r, spans, g)
    y = _C().nf4_gemv(x, q, a, N, K, h, Bs, offs, SCALING)
    _check(y, y64, mag + lmag, K + r, f"nf4_gemv+lora {M}x{N}x{K} r={r}")
    # the h column blocks follow the list order, not the row order
    if len(spans) > 1:
        perm = list(reversed(range(len(spans))))
        hp = torch.cat([h[:, i * r:(i + 1) * r] for i in perm], 1).contiguous()
        yp = _C().nf4_gemv(x, q, a, N, K, hp, [Bs[i] for i in perm], [offs[i] for i in perm], SCALING)
        assert torch.equal(y, yp)


# ------------------------------------------------------------------ 3. bitwise stability
def test_bitwise_stable_and_no_stale_lds():
    C = _C()
    g = _gen(3)
    x, q, a, h, Bs, offs, *_ = _lora_case(2, 768, 256, 16, [(0, 256), (512, 256)], g)
    q2, a2, _ = _weights(64, 8192, g)
    x2 = _x(1, 8192, g, False)
    dev = torch.cuda.current_device()

    def run():
        return C.nf4_gemv(x, q, a, 768, 256, h, Bs, offs, SCALING), C.nf4_gemv(x2, q2, a2, 64, 8192)

    first, second = run(), run()
    for u, v in zip(first, second):
        assert torch.equal(u, v), "two calls differ"
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    for pat in (QNAN, 0):
        C.lds_fill(pat, dev)
        ya = C.nf4_gemv(x, q, a, 768, 256, h, Bs, offs, SCALING)
        C.lds_fill(pat, dev)
        yb = C.nf4_gemv(x2, q2, a2, 64, 8192)
        torch.cuda.synchronize()
        assert torch.equal(ya, first[0]) and torch.equal(yb, first[1]), f"stale LDS read (pattern {pat:#x})"


# ------------------------------------------------------------------ 4. binding guards
def test_binding_guards():
    C = _C()
    g = _gen(4)
    N, K = 16, 128
    q, a, _ = _weights(N, K, g)
    x = _x(2, K, g, False)
    h = torch.zeros(2, 8, device=DEV, dtype=torch.bfloat16)
    b = torch.zeros(8, 8, device=DEV, dtype=torch.bfloat16)
    assert C.nf4_gemv(x, q, a, N, K, h, [b], [4], 1.0).shape == (2, N)  # the baseline call is valid
    with pytest.raises(RuntimeError, match="rows"):
        C.nf4_gemv(_x(5, K, g, False), q, a, N, K)
    q96, a96 = torch.zeros(N * 96 // 2, device=DEV, dtype=torch.uint8), torch.ones(N * 96 // 64, device=DEV)
    with pytest.raises(RuntimeError, match="K % 64"):
        C.nf4_gemv(_x(2, 96, g, False), q96, a96, N, 96)
    with pytest.raises(RuntimeError, match="bf16"):
        C.nf4_gemv(x.float(), q, a, N, K)
    with pytest.raises(RuntimeError, match="shapes"):
        C.nf4_gemv(x, q, a[:-1].contiguous(), N, K)
    with pytest.raises(RuntimeError, match="lora_off"):
        C.nf4_gemv(x, q, a, N, K, h, [b], [2], 1.0)
    h72 = torch.zeros(2, 72, device=DEV, dtype=torch.bfloat16)
    b72 = torch.zeros(8, 72, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="r <= 64"):
        C.nf4_gemv(x, q, a, N, K, h72, [b72], [4], 1.0)
    with pytest.raises(RuntimeError, match="targets"):
        C.nf4_gemv(x, q, a, N, K, torch.zeros(2, 40, device=DEV, dtype=torch.bfloat16), [b] * 5, [0] * 5, 1.0)
    with pytest.raises(RuntimeError, match="overlap"):
        C.nf4_gemv(x, q, a, N, K, torch.zeros(2, 16, device=DEV, dtype=torch.bfloat16), [b, b], [0, 4], 1.0)
    with pytest.raises(RuntimeError, match="inside"):
        C.nf4_gemv(x, q, a, N, K, h, [b], [12], 1.0)


# ------------------------------------------------------------------ 5. modules
def _nf4_linear(K, N, double_quant, g):
    from gke_ray_train_amd.peft.quant import BitsAndBytesConfig, NF4Linear
    lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, device=DEV, generator=g) * 0.05)
    m = NF4Linear.from_linear(lin, BitsAndBytesConfig(bnb_4bit_use_double_quant=double_quant))
    m.set_dequant_cache(False)
    return m.eval()


def _lora_on(base, spans, r, g):
    from gke_ray_train_amd.peft.lora import LoraConfig, LoraLinear
    lw = LoraLinear(base, [(f"t{i}_proj", off, n) for i, (off, n) in enumerate(spans)],
                    LoraConfig(r=r, lora_alpha=int(SCALING * r), lora_dropout=0.1))
    with torch.no_grad():
        for p in lw.lora_B.values():
            p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.05)
    return lw.eval()


def _module_w32(m):
    from gke_ray_train_amd.ops import _ref
    return _ref.nf4_dequantize(m.qweight, m._absmax().contiguous(), m.in_features * m.out_features, 64,
                               torch.float32).view(m.out_features, m.in_features)


def _old_nf4(m, x):
    return torch.nn.functional.linear(x, m.dequantize())


def _old_lora(lw, x):
    from gke_ray_train_amd.peft.lora import _LoraFn
    names = [t[0] for t in lw.targets]
    return _LoraFn.apply(x, lw.base, [(off, n) for _, off, n in lw.targets], lw.r, lw.scaling, 0.0, 0, 0,
                         *[lw.lora_A[n] for n in names], *[lw.lora_B[n] for n in names])


@pytest.mark.parametrize("double_quant", [False, True])
@pytest.mark.parametrize("rows", [1, 2])
def test_modules_match_float64(double_quant, rows):
    g = _gen(50 + rows + 2 * double_quant)
    K, N, r = 512, 768, 16
    spans = [(0, 512), (512, 128), (640, 128)]
    base = _nf4_linear(K, N, double_quant, g)
    lw = _lora_on(base, spans, r, g)
    assert lw.scaling == SCALING
    x = _x(rows, K, g, False)
    w32 = _module_w32(base).double()
    y64 = x.double() @ w32.t()
    mag = x.double().abs() @ w32.abs().t()
    with torch.no_grad():
        y = base(x)
        yl = lw(x)
    _check(y, y64, mag, K, f"NF4Linear dq={double_quant} rows={rows}")
    lmag = torch.zeros_like(mag)
    for i, (off, n) in enumerate(spans):
        h64 = x.double() @ lw.lora_A[f"t{i}_proj"].double().t()
        b = lw.lora_B[f"t{i}_proj"].double()
        y64[:, off:off + n] += SCALING * (h64 @ b.t())
        lmag[:, off:off + n] += SCALING * (h64.abs() @ b.abs().t())
    _check(yl, y64, mag + lmag, K + r, f"LoraLinear dq={double_quant} rows={rows}", extra=2.0 ** -7 * lmag)
    if double_quant:  # the expanded absmax is kept, and is what _absmax() gives
        assert base._absmax_cache[1] is base._absmax_f32()
        assert torch.equal(base._absmax_f32(), base._absmax().contiguous())
        assert "_absmax_cache" not in base.state_dict() and len(base.state_dict()) == 4


def _unchanged_cases():
    """(what, module output, the path every call took before the kernel existed) for inputs the kernel
    must not take: 5 rows, and in_features = 688 (not a multiple of 64)."""
    g = _gen(60)
    out = []
    for what, K, rows in (("5 rows", 512, 5), ("K = 688", 688, 1)):
        base = _nf4_linear(K, 256, False, g)
        lw = _lora_on(base, [(0, 128), (128, 128)], 8, g)
        x = _x(rows, K, g, False)
        with torch.no_grad():
            out.append((f"NF4Linear, {what}", base(x), _old_nf4(base, x)))
            out.append((f"LoraLinear, {what}", lw(x), _old_lora(lw, x)))
    return out


def test_modules_unchanged_outside_the_kernels_domain(monkeypatch):
    from gke_ray_train_amd import ops
    calls = []
    monkeypatch.setattr(ops, "nf4_gemv", lambda *a, **k: calls.append(1))
    for what, got, want in _unchanged_cases():
        assert torch.equal(got, want), what
    assert not calls


def _child():
    """GRT_NF4_GEMV=0 (read at import): kernel-sized inputs take the dequantising path."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.peft import quant
    assert not quant._NF4_GEMV
    calls = []
    real = ops.nf4_gemv
    ops.nf4_gemv = lambda *a, **k: calls.append(1) or real(*a, **k)
    g = _gen(70)
    base = _nf4_linear(512, 256, False, g)
    lw = _lora_on(base, [(0, 128), (128, 128)], 8, g)
    for rows in (1, 2):
        x = _x(rows, 512, g, False)
        with torch.no_grad():
            assert torch.equal(base(x), _old_nf4(base, x))
            assert torch.equal(lw(x), _old_lora(lw, x))
    assert not calls, "the NF4 GEMV ran with GRT_NF4_GEMV=0"
    print("child ok")


def test_switch_off_in_child():
    env = dict(os.environ, GRT_NF4_GEMV="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, f"child exited with {r.returncode}:\n{r.stdout}"


# ------------------------------------------------------------------ 6. routing
def _qlora_model(name, cache, **overrides):
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    from gke_ray_train_amd.peft.quant import set_dequant_cache
    m = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=0, **overrides)
    quantize_model_(m, BitsAndBytesConfig())
    if cache is not None:
        set_dequant_cache(m, cache)
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16))
    g = _gen(6)
    with torch.no_grad():
        for lw in pm.lora_modules.values():
            for p in lw.lora_B.values():
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.05)
    assert len(pm.lora_modules) == 4 * m.config.num_hidden_layers  # qkv, o, gate_up, down: all 7 targets
    return pm.eval()


def test_decode_never_dequantises(monkeypatch):
    """This is the test that fails without the kernel: with the dequant cache off, every decode
    step of a QLoRA model used to dequantise every projection."""
    from gke_ray_train_amd.models.generation import GraphDecoder, KVCache, forward_cached
    from gke_ray_train_amd.peft.quant import NF4Linear
    pm = _qlora_model("llama-tiny-gqa", "0", intermediate_size=1536)
    model = pm.base_model
    ids = torch.randint(0, 512, (1, 40), device=DEV, generator=_gen(61))
    dec = GraphDecoder(model, 1, 64)
    logits = dec.prefill(ids)
    cache = KVCache(model.config, 1, 64, ids.device, torch.bfloat16)
    elogits = forward_cached(model, ids, cache)
    count = {"n": 0}
    for name in ("_dequant", "dequantize_into", "_dequant_t"):
        real = getattr(NF4Linear, name)

        def counted(self, *a, _real=real, **k):
            count["n"] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(NF4Linear, name, counted)
    for _ in range(8):
        logits = dec.step(logits.argmax(-1))
    torch.cuda.synchronize()
    assert count["n"] == 0, f"{count['n']} dequantisations in 8 graph decode steps"
    assert torch.isfinite(logits).all()
    for _ in range(8):
        elogits = forward_cached(model, elogits.argmax(-1)[:, None], cache)
    assert count["n"] == 0, f"{count['n']} dequantisations in 8 eager decode steps"
    forward_cached(model, ids[:, :8], KVCache(model.config, 1, 64, ids.device, torch.bfloat16))
    assert count["n"] > 0  # the counters do count: an 8-row prefill dequantises


# ------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("name,inter", [("llama-tiny-gqa", 1536), ("llama-tiny-d64", 768)])
def test_generate_from_nf4_base(name, inter):
    pm = _qlora_model(name, None, intermediate_size=inter)
    ids = torch.randint(0, 512, (2, 40), device=DEV, generator=_gen(7))
    P, T = 40, 8
    out = pm.generate(ids, max_new_tokens=T, use_graph=True)
    eager = pm.generate(ids, max_new_tokens=T, use_graph=False)
    assert out.shape == (2, P + T) and torch.equal(out[:, :P], ids)
    assert torch.equal(out, eager), (out[:, P:], eager[:, P:])
    # teacher-forced, as tests/test_gpu_jobs.py test_generation_cache_matches_recompute: the
    # full-recompute logits (94 rows: the dequantising path) pick each generated token or tie with it
    with torch.no_grad():
        lg = pm(out[:, :-1], return_logits=True)["logits"][:, P - 1:].float()
    gen = out[:, P:]
    best = lg.max(-1).values
    got = lg.gather(-1, gen.unsqueeze(-1)).squeeze(-1)
    tol = 0.02 + 0.01 * best.abs()
    assert bool((got >= best - tol).all()), (best - got).max().item()
    assert (lg.argmax(-1) == gen).float().mean().item() > 0.8


def test_generate_with_mixed_kernel_and_fallback_layers():
    """llama-tiny-gqa as it is: the down projection's K = 1376 is no multiple of 64, so it
    dequantises while every other projection runs from the codes, eagerly and under capture."""
    pm = _qlora_model("llama-tiny-gqa", "0")
    ids = torch.randint(0, 512, (2, 40), device=DEV, generator=_gen(8))
    out = pm.generate(ids, max_new_tokens=4, use_graph=True)
    eager = pm.generate(ids, max_new_tokens=4, use_graph=False)
    assert out.shape == (2, 44) and torch.equal(out, eager), (out[:, 40:], eager[:, 40:])


if __name__ == "__main__":
    if sys.argv[1:] != ["--child"]:
        sys.exit("usage: test_nf4_gemv_gpu.py --child (started by test_switch_off_in_child)")
    _child()
