"""bf16 flash attention at head_dim 64 (csrc/kernels/attention_d64.hip) against the fp32 math path,
from the raw binding up to the models that run on it (llama-tiny-d64, BasicLLM's attention site)."""
import contextlib
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
QNAN = 0x7FC00000
TOL_O, TOL_G = 2e-2, 3e-2  # the project's bf16 attention tolerances (tests/test_kernels_gpu.py)


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _close(a, b, atol, rtol, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not torch.isnan(a).any(), f"{what}: NaN in kernel output"
    assert bad.float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    # no element may be far off: a wrong row / tile edge fails even if it is < 0.1 % of the tensor
    worst = (err / tol).max().item()
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"


def _inputs(B, Sq, Sk, Hq, Hkv, strided=False, D=D, dtype=torch.bfloat16):
    torch.manual_seed(8)
    if strided:
        qkv = torch.randn(B, Sq, Hq + 2 * Hkv, D, device=DEV, dtype=dtype)
        q = qkv[:, :, :Hq].detach().requires_grad_()
        base = torch.randn(B, Sk, 2 * Hkv, D, device=DEV, dtype=dtype)
        k = base[:, :, :Hkv].detach().requires_grad_()
        v = base[:, :, Hkv:].detach().requires_grad_()
    else:
        q = torch.randn(B, Sq, Hq, D, device=DEV, dtype=dtype, requires_grad=True)
        k = torch.randn(B, Sk, Hkv, D, device=DEV, dtype=dtype, requires_grad=True)
        v = torch.randn(B, Sk, Hkv, D, device=DEV, dtype=dtype, requires_grad=True)
    return q, k, v


def _attn_case(B, Sq, Sk, Hq, Hkv, causal, seqlens=None, strided=False, dropout_p=0.0, dtype=torch.bfloat16, D=D):
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    q, k, v = _inputs(B, Sq, Sk, Hq, Hkv, strided, D, dtype)
    sl = None if seqlens is None else torch.tensor(seqlens, device=DEV, dtype=torch.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the fp32 math fallback announces itself with a warning
        o = ops.flash_attention(q, k, v, causal=causal, seqlens_k=sl, dropout_p=dropout_p, seed=1234)
    do = torch.randn_like(o)
    (o.float() * do.float()).sum().backward()
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    orf = _ref.attention(qr, kr, vr, causal=causal, seqlens_k=sl, dropout_p=dropout_p, seed=1234)
    (orf * do.float()).sum().backward()
    _close(o, orf, TOL_O, TOL_O, "attn o")
    _close(q.grad, qr.grad, TOL_G, TOL_G, "attn dq")
    _close(k.grad, kr.grad, TOL_G, TOL_G, "attn dk")
    _close(v.grad, vr.grad, TOL_G, TOL_G, "attn dv")


@contextlib.contextmanager
def _no_fallback(monkeypatch):
    """Any warning is an error and the fp32 math attention raises: only the kernels may run."""
    from gke_ray_train_amd.ops import _ref

    def boom(*a, **k):
        raise AssertionError("fp32 math attention path used")
    with monkeypatch.context() as mp, warnings.catch_warnings():
        warnings.simplefilter("error")
        mp.setattr(_ref, "attention", boom)
        yield


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", [
    dict(B=2, Sq=256, Sk=256, Hq=4, Hkv=4, causal=True),
    dict(B=1, Sq=200, Sk=200, Hq=4, Hkv=2, causal=True),                          # partial last tile, GQA
    dict(B=2, Sq=130, Sk=130, Hq=2, Hkv=2, causal=False),                         # 2 rows into a second block
    dict(B=1, Sq=64, Sk=192, Hq=2, Hkv=1, causal=True),                           # Sk > Sq, bottom-right offset
    dict(B=2, Sq=256, Sk=256, Hq=4, Hkv=2, causal=True, strided=True),
    dict(B=2, Sq=160, Sk=160, Hq=2, Hkv=2, causal=False, seqlens=[160, 77]),      # mask ends inside a tile
    dict(B=2, Sq=256, Sk=256, Hq=4, Hkv=2, causal=True, dropout_p=0.1),
    dict(B=1, Sq=200, Sk=200, Hq=2, Hkv=2, causal=True, dropout_p=0.3),
    dict(B=3, Sq=1, Sk=97, Hq=4, Hkv=2, causal=False, seqlens=[97, 40, 1]),       # generation.py's decode call
])
def test_flash_attention_d64(case):
    _attn_case(**case)


def test_flash_attention_d64_decode_no_grad():
    """One query token over a right-padded cache under no_grad: the forward kernel, not the
    head_dim-128 split-K decode kernel."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    q, k, v = _inputs(3, 1, 97, 4, 2)
    sl = torch.tensor([97, 40, 1], device=DEV, dtype=torch.int32)
    orf = _ref.attention(q.detach().float(), k.detach().float(), v.detach().float(), causal=False, seqlens_k=sl)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")
        o = ops.flash_attention(q, k, v, causal=False, seqlens_k=sl)
    _close(o, orf, TOL_O, TOL_O, "decode o")


# ------------------------------------------------------------------ 2. fully masked rows
def test_fully_masked_rows():
    from gke_ray_train_amd.ops import _ref
    C = _C()
    q, k, v = (t.detach() for t in _inputs(2, 64, 64, 2, 2))
    do = torch.randn_like(q)
    sl = torch.tensor([64, 0], device=DEV, dtype=torch.int32)
    o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, False, sl)
    dq, dk, dv = C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, False, sl)
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t.float()).all(), f"{name}: non-finite"
        assert (t[1] == 0).all(), f"{name}: batch with no valid key must be zero"
    assert torch.isinf(lse[1]).all() and (lse[1] > 0).all() and torch.isfinite(lse[0]).all()
    qr, kr, vr = (t[:1].float().requires_grad_() for t in (q, k, v))
    orf = _ref.attention(qr, kr, vr, causal=False)
    (orf * do[:1].float()).sum().backward()
    _close(o[:1], orf, TOL_O, TOL_O, "o batch 0")
    _close(dq[:1], qr.grad, TOL_G, TOL_G, "dq batch 0")
    _close(dk[:1], kr.grad, TOL_G, TOL_G, "dk batch 0")
    _close(dv[:1], vr.grad, TOL_G, TOL_G, "dv batch 0")


# ------------------------------------------------------------------ 3. direct binding
def test_direct_binding():
    from gke_ray_train_amd.ops import _ref
    C = _C()
    q, k, v = (t.detach() for t in _inputs(2, 96, 96, 4, 4))
    do = torch.randn_like(q)
    o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, True, None)
    dq, dk, dv = C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None)
    assert o.dtype == torch.bfloat16 and lse.shape == (2, 4, 96) and lse.dtype == torch.float32
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    orf = _ref.attention(qr, kr, vr, causal=True)
    (orf * do.float()).sum().backward()
    s = torch.einsum("bqhd,bkhd->bhqk", qr.detach(), kr.detach()) * D ** -0.5
    s = s.masked_fill(torch.ones(96, 96, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    _close(lse, torch.logsumexp(s, -1), 2e-2, 2e-2, "lse")
    _close(o, orf, TOL_O, TOL_O, "o")
    _close(dq, qr.grad, TOL_G, TOL_G, "dq")
    _close(dk, kr.grad, TOL_G, TOL_G, "dk")
    _close(dv, vr.grad, TOL_G, TOL_G, "dv")


# ------------------------------------------------------------------ 4. no fallback
def test_flash_attention_no_fallback(monkeypatch):
    from gke_ray_train_amd import ops
    q, k, v = _inputs(2, 96, 96, 4, 2)
    with _no_fallback(monkeypatch):
        o = ops.flash_attention(q, k, v, causal=True)
        o.float().sum().backward()
        torch.cuda.synchronize()
    assert all(torch.isfinite(t.grad.float()).all() for t in (q, k, v))


def test_rope_attention_no_fallback(monkeypatch):
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    B, S, hq, hkv = 2, 96, 4, 2
    torch.manual_seed(9)
    qkv = torch.randn(B * S, (hq + 2 * hkv) * D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    cos, sin = _ref.rope_tables(S, D, 10000.0, device=DEV)
    g = torch.randn(B * S, hq * D, device=DEV, dtype=torch.bfloat16)
    xr = qkv.detach().float().requires_grad_()
    x = xr.view(B * S, hq + 2 * hkv, D)
    qf = _ref.apply_rope(x[:, :hq], cos, sin).view(B, S, hq, D)
    kf = _ref.apply_rope(x[:, hq:hq + hkv], cos, sin).view(B, S, hkv, D)
    vf = x[:, hq + hkv:].reshape(B, S, hkv, D)
    orf = _ref.attention(qf, kf, vf, causal=True).reshape(B * S, hq * D)
    (orf * g.float()).sum().backward()
    with _no_fallback(monkeypatch):
        o = ops.rope_attention(qkv, cos, sin, B, S, hq, hkv, D)
        (o.float() * g.float()).sum().backward()
        torch.cuda.synchronize()
    _close(o, orf, TOL_O, TOL_O, "rope-attn o")
    _close(qkv.grad, xr.grad, TOL_G, TOL_G, "rope-attn dqkv")


# ------------------------------------------------------------------ 5. unsupported combinations
def test_d128_only_features_refused_at_d64():
    C = _C()
    T, H = 96, 2
    q, k, v = (torch.randn(1, T, H, D, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    cu = torch.tensor([0, 40, T], device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_fwd(q, k, v, None, D ** -0.5, True, None, cu_seqlens=cu, max_seqlen=56)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_fwd(q, k, v, None, D ** -0.5, True, None,
                   o_t=torch.empty(H * D, T, device=DEV, dtype=torch.bfloat16))
    o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, True, None)
    do = torch.randn_like(q)
    cos = torch.ones(T, D // 2, device=DEV)
    sin = torch.zeros(T, D // 2, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None, rope_cos=cos, rope_sin=sin)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None,
                   dqkv_t=torch.empty(3 * H * D, T, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_decode(q[:, :1], k, v, None, D ** -0.5)
    torch.cuda.synchronize()


def test_d96_still_falls_back_with_warning(monkeypatch):
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    from gke_ray_train_amd.ops import fused as F_
    monkeypatch.setattr(F_, "_warned", set())
    q, k, v = _inputs(1, 40, 40, 2, 2, D=96)
    with pytest.warns(UserWarning, match="no gfx950 kernel.*head_dim=96"):
        o = ops.flash_attention(q, k, v, causal=True)
    assert torch.equal(o, _ref.attention(q, k, v, causal=True))
    with pytest.raises(RuntimeError, match="head_dim 64 or 128"):
        _C().attn_fwd(q.detach(), k.detach(), v.detach(), None, 96 ** -0.5, True, None)


# ------------------------------------------------------------------ 6. determinism
def test_dropout_case_is_bitwise_repeatable():
    C = _C()
    q, k, v = (t.detach() for t in _inputs(2, 256, 256, 4, 2))
    do = torch.randn_like(q)
    res = []
    for _ in range(2):
        o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, True, None, 0.1, 1234)
        dq, dk, dv = C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None, 0.1, 1234)
        torch.cuda.synchronize()
        res.append((o, lse, dq, dk, dv))
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(x, y), f"{name}: two runs differ"


# ------------------------------------------------------------------ 7. stale LDS
@pytest.mark.parametrize("B,S,Hq,Hkv,dropout_p", [(2, 128, 4, 2, 0.0), (2, 300, 8, 2, 0.0), (2, 300, 8, 2, 0.1)])
def test_attention_d64_reads_no_stale_lds(B, S, Hq, Hkv, dropout_p):
    C = _C()
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    dev = torch.cuda.current_device()
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    res = []
    for pat in (QNAN, 0):
        C.lds_fill(pat, dev)
        o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, True, None, dropout_p, 7)
        C.lds_fill(pat, dev)
        dq, dk, dv = C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None, dropout_p, 7)
        torch.cuda.synchronize()
        res.append((o, lse, dq, dk, dv))
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), *res):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y), f"{name}: stale LDS read (B{B} S{S} Hq{Hq} Hkv{Hkv})"


# ------------------------------------------------------------------ 8. D = 128 untouched
def test_d128_dispatch_unchanged():
    _attn_case(B=2, Sq=256, Sk=256, Hq=4, Hkv=4, causal=True, D=128)


# ------------------------------------------------------------------ 9. model level
def test_llama_tiny_d64_matches_reference_math(monkeypatch):
    from gke_ray_train_amd.models import build_llama
    torch.manual_seed(10)
    m = build_llama("llama-tiny-d64", device=DEV, dtype=torch.bfloat16, seed=1)
    assert m.config.head_dim == 64
    ids = torch.randint(0, m.config.vocab_size, (2, 128), device=DEV)
    with _no_fallback(monkeypatch):
        loss = m(ids, labels=ids)["loss"]
        loss.backward()
        torch.cuda.synchronize()
    g_native = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    mc = build_llama("llama-tiny-d64", device="cpu", dtype=torch.float32, seed=None)
    mc.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    lc = mc(ids.cpu(), labels=ids.cpu())["loss"]
    lc.backward()
    assert abs(loss.item() - lc.item()) < 2e-2 * max(1.0, lc.item())
    for n, p in mc.named_parameters():
        a, b = g_native[n].cpu(), p.grad
        rel = (a - b).norm() / (b.norm() + 1e-8)
        assert rel < 0.08, f"{n}: rel grad err {rel:.3f}"


# ------------------------------------------------------------------ 10. BasicLLM attention site
def test_basic_llm_mha_site():
    """_MHA slices q / k / v out of a [B, S, 3, H, 64] projection (strided views) and drops
    attention probabilities; bf16 on the head_dim-64 kernels vs the same weights in fp32 on the
    exact-fp32 kernels, same dropout seed."""
    from gke_ray_train_amd.models.basic_llm import _MHA
    B, S, d = 2, 96, 128
    torch.manual_seed(3)
    mb = _MHA(d, 2, 0.1, device=DEV, dtype=torch.bfloat16)
    mf = _MHA(d, 2, 0.1, device=DEV, dtype=torch.float32)
    mf.load_state_dict({k: v.float() for k, v in mb.state_dict().items()})
    xb = torch.randn(B * S, d, device=DEV, dtype=torch.bfloat16).requires_grad_()
    xf = xb.detach().float().requires_grad_()
    g = torch.randn(B * S, d, device=DEV, dtype=torch.bfloat16)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        torch.manual_seed(21)
        yb = mb(xb, B, S, True)
        (yb.float() * g.float()).sum().backward()
        torch.manual_seed(21)
        yf = mf(xf, B, S, True)
        (yf * g.float()).sum().backward()
    _close(yb, yf, TOL_O, TOL_O, "mha out")
    _close(xb.grad, xf.grad, TOL_G, TOL_G, "mha dx")
