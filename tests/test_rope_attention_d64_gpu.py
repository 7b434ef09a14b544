"""Fused RoPE + packed flash attention at head_dim 64 on the fused QKV buffer
(the FusedRope kernels of csrc/kernels/attention_d64.hip): the raw bindings, ``ops.rope_attention`` and llama-tiny-d64
against the fp32 math path run sequence by sequence (``_ref.apply_rope`` with the positions of
``Varlen.pos``, then ``_ref.attention``)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
QNAN = 0x7FC00000
TOL_O, TOL_G = 2e-2, 3e-2  # the project's bf16 attention tolerances (tests/test_attention_d64_gpu.py)
# length 1, one past a tile, one past a 128-row block, an exact multiple of the tile, two blocks
LENS = [1, 33, 129, 64, 200]


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


def _reference(qkv, do, cos, sin, hq, hkv, pos, bounds, causal):
    """fp32: rotate with ``pos``, attention over each [a, b) row range alone -> (o, dqkv)."""
    from gke_ray_train_amd.ops import _ref
    T = qkv.shape[0]
    x = qkv.detach().float().requires_grad_()
    xr = x.view(T, hq + 2 * hkv, D)
    q = _ref.apply_rope(xr[:, :hq], cos, sin, pos)
    k = _ref.apply_rope(xr[:, hq:hq + hkv], cos, sin, pos)
    v = xr[:, hq + hkv:]
    outs = [_ref.attention(q[a:b].unsqueeze(0), k[a:b].unsqueeze(0), v[a:b].unsqueeze(0), causal=causal)[0]
            for a, b in bounds]
    ref = torch.cat(outs).reshape(T, hq * D)
    (ref * do.float()).sum().backward()
    return ref.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _packed(hq, hkv):
    """One packed problem per head layout, with its fp32 reference; shared, never modified."""
    from gke_ray_train_amd.ops import Varlen, _ref
    torch.manual_seed(1)
    vl = Varlen(LENS, torch.device(DEV, 0))
    T = vl.total
    qkv = torch.randn(T, (hq + 2 * hkv) * D, device=DEV, dtype=torch.bfloat16)
    do = torch.randn(T, hq * D, device=DEV, dtype=torch.bfloat16)
    cos, sin = _ref.rope_tables(vl.max_len, D, device=DEV)
    bounds = list(zip(vl.cu_host[:-1], vl.cu_host[1:]))
    ref_o, ref_g = _reference(qkv, do, cos, sin, hq, hkv, vl.pos, bounds, True)
    return vl, qkv, do, cos, sin, ref_o, ref_g


def _raw(qkv, do, cos, sin, hq, hkv, B, S, cu=None, ml=0, causal=True, pad=0, fill=None):
    """The two bindings on their own buffers -> (o rows buffer [T, Hq*64 + pad], lse, dqkv)."""
    C = _C()
    T = qkv.shape[0]
    ld = hq * D + pad
    buf = torch.empty(T, ld, device=DEV, dtype=torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    if fill is not None:
        buf.fill_(fill)
        dqkv.fill_(float("nan"))
    o = buf.as_strided((T, hq, D), (ld, D, 1))
    lse = C.rope_attn_fwd_d64(qkv, cos, sin, o, B, S, hq, hkv, D ** -0.5, causal, cu_seqlens=cu, max_seqlen=ml)
    C.rope_attn_bwd_d64(do, qkv, cos, sin, o, lse, dqkv, B, S, hq, hkv, D ** -0.5, causal, cu_seqlens=cu,
                        max_seqlen=ml)
    torch.cuda.synchronize()
    return buf, lse, dqkv


def _op_parity(hq, hkv):
    from gke_ray_train_amd import ops
    vl, qkv, do, cos, sin, ref_o, ref_g = _packed(hq, hkv)
    x = qkv.clone().requires_grad_()
    o = ops.rope_attention(x, cos, sin, 1, vl.total, hq, hkv, D, causal=True, varlen=vl)
    (o.float() * do.float()).sum().backward()
    torch.cuda.synchronize()
    assert o.shape == (vl.total, hq * D) and x.grad.shape == qkv.shape
    _close(o, ref_o, TOL_O, TOL_O, "packed o")
    _close(x.grad, ref_g, TOL_G, TOL_G, "packed dqkv")


# ------------------------------------------------------------------ 1. parity, packed
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_packed_matches_fp32_per_sequence(hq, hkv, monkeypatch):
    from gke_ray_train_amd.ops import fused

    def boom(*a, **k):
        raise AssertionError("rope_attention left the qkv-native kernels")
    monkeypatch.setattr(fused, "flash_attention", boom)
    _op_parity(hq, hkv)


# ------------------------------------------------------------------ 2. parity, unpacked
@pytest.mark.parametrize("B,S,causal", [(2, 96, True), (1, 200, True), (2, 96, False)])
def test_unpacked_matches_fp32(B, S, causal):
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    hq, hkv = 4, 2
    torch.manual_seed(2)
    T = B * S
    qkv = torch.randn(T, (hq + 2 * hkv) * D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(T, hq * D, device=DEV, dtype=torch.bfloat16)
    cos, sin = _ref.rope_tables(S, D, device=DEV)
    pos = torch.arange(T, device=DEV) % S
    ref_o, ref_g = _reference(qkv, do, cos, sin, hq, hkv, pos, [(b * S, (b + 1) * S) for b in range(B)], causal)
    o = ops.rope_attention(qkv, cos, sin, B, S, hq, hkv, D, causal=causal)
    (o.float() * do.float()).sum().backward()
    torch.cuda.synchronize()
    _close(o, ref_o, TOL_O, TOL_O, "o")
    _close(qkv.grad, ref_g, TOL_G, TOL_G, "dqkv")


# ------------------------------------------------------------------ 3. packed == one by one, bitwise
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_packed_equals_each_sequence_alone_bitwise(hq, hkv):
    """Tiles are aligned to each sequence's start and nothing is atomic: any difference is one
    sequence reading or writing another's rows."""
    vl, qkv, do, cos, sin, _, _ = _packed(hq, hkv)
    o, lse, dqkv = _raw(qkv, do, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len)
    assert lse.shape == (len(LENS), hq, vl.max_len) and lse.dtype == torch.float32
    cols = {"dq": slice(0, hq * D), "dk": slice(hq * D, (hq + hkv) * D), "dv": slice((hq + hkv) * D, None)}
    for i, (a, b) in enumerate(zip(vl.cu_host[:-1], vl.cu_host[1:])):
        n = b - a
        o1, lse1, g1 = _raw(qkv[a:b], do[a:b], cos, sin, hq, hkv, 1, n)
        assert lse1.shape == (1, hq, n)
        assert torch.equal(o[a:b], o1), f"o of sequence {i} (len {n})"
        assert torch.equal(lse[i, :, :n], lse1[0]), f"lse of sequence {i} (len {n})"
        for name, c in cols.items():
            assert torch.equal(dqkv[a:b, c], g1[:, c]), f"{name} of sequence {i} (len {n})"


# ------------------------------------------------------------------ 4. neighbours are invisible
def test_other_sequences_rows_are_never_read():
    hq, hkv, i = 8, 2, 2
    vl, qkv, do, cos, sin, _, _ = _packed(hq, hkv)
    a, b = vl.cu_host[i], vl.cu_host[i + 1]
    o, _, dqkv = _raw(qkv, do, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len)
    qkv_n = torch.full_like(qkv, float("nan"))
    do_n = torch.full_like(do, float("nan"))
    qkv_n[a:b] = qkv[a:b]
    do_n[a:b] = do[a:b]
    o_n, _, dqkv_n = _raw(qkv_n, do_n, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len)
    for name, x, y in (("o", o, o_n), ("dqkv", dqkv, dqkv_n)):
        assert torch.isfinite(y[a:b].float()).all(), f"{name}: NaN from a neighbouring sequence"
        assert torch.equal(x[a:b], y[a:b]), f"{name}: depends on a neighbouring sequence's rows"


# ------------------------------------------------------------------ 5. tail columns, full dqkv
def test_tail_columns_kept_and_dqkv_fully_written():
    from gke_ray_train_amd import ops
    hq, hkv, pad, sentinel = 4, 4, 64, 7.0
    vl, qkv, do, cos, sin, ref_o, _ = _packed(hq, hkv)
    buf, _, dqkv = _raw(qkv, do, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len, pad=pad, fill=sentinel)
    assert (buf[:, hq * D:] == sentinel).all(), "the tail columns after each output row were written"
    _close(buf[:, :hq * D], ref_o, TOL_O, TOL_O, "o in a padded row buffer")
    assert torch.isfinite(dqkv.float()).all(), "an element of dqkv was not written"
    x = qkv.clone().requires_grad_()
    o = ops.rope_attention(x, cos, sin, 1, vl.total, hq, hkv, D, causal=True, varlen=vl, pad=pad)
    assert getattr(o, "_grt_tail", None) == pad
    assert o.shape == (vl.total, hq * D) and o.stride() == (hq * D + pad, 1)
    assert not hasattr(o, "_grt_T")
    assert torch.equal(o, buf[:, :hq * D])
    (o.float() * do.float()).sum().backward()
    assert torch.equal(x.grad, dqkv)


# ------------------------------------------------------------------ 6. stale LDS
def test_reads_no_stale_lds():
    C = _C()
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    hq, hkv = 8, 2
    vl, qkv, do, cos, sin, _, _ = _packed(hq, hkv)
    dev = torch.cuda.current_device()
    T = vl.total
    res = []
    for pat in (QNAN, 0):
        o = torch.empty(T, hq, D, device=DEV, dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        C.lds_fill(pat, dev)
        lse = C.rope_attn_fwd_d64(qkv, cos, sin, o, 1, T, hq, hkv, D ** -0.5, True, cu_seqlens=vl.cu,
                                  max_seqlen=vl.max_len)
        C.lds_fill(pat, dev)
        C.rope_attn_bwd_d64(do, qkv, cos, sin, o, lse, dqkv, 1, T, hq, hkv, D ** -0.5, True, cu_seqlens=vl.cu,
                            max_seqlen=vl.max_len)
        torch.cuda.synchronize()
        res.append((o, dqkv))
    for name, x, y in zip(("o", "dqkv"), *res):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y), f"{name}: stale LDS read"


# ------------------------------------------------------------------ 7. determinism
def test_packed_runs_are_bitwise_repeatable():
    hq, hkv = 8, 2
    vl, qkv, do, cos, sin, _, _ = _packed(hq, hkv)
    r1 = _raw(qkv, do, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len)
    r2 = _raw(qkv, do, cos, sin, hq, hkv, 1, vl.total, vl.cu, vl.max_len)
    for name, x, y in zip(("o", "lse", "dqkv"), r1, r2):
        if name == "lse":  # rows past a sequence's end are not written
            for i, n in enumerate(LENS):
                assert torch.equal(x[i, :, :n], y[i, :, :n]), "lse: two runs differ"
        else:
            assert torch.equal(x, y), f"{name}: two runs differ"


# ------------------------------------------------------------------ 7b. one kernel, two entry points
@pytest.mark.parametrize("B,S,hq,hkv,causal", [(2, 200, 8, 2, True), (1, 33, 4, 4, True), (2, 96, 4, 2, False)])
def test_identity_rotation_equals_the_plain_kernels(B, S, hq, hkv, causal):
    """attention_d64.hip writes each kernel once for both sources, so with cos = 1, sin = 0 the
    qkv-native entry points must give the values of attn_fwd / attn_bwd on the q, k, v column
    views of the same buffer: own * 1 -+ partner * 0 rounds back to the bf16 it came from,
    a0 * 1 + a1 * 0 is a0 in fp32, and all other arithmetic is shared (finite inputs keep
    partner * 0 from being NaN). torch.equal compares values, so a zero's sign does not count."""
    C = _C()
    torch.manual_seed(4)
    T, W, sc = B * S, (hq + 2 * hkv) * D, D ** -0.5
    qkv = torch.randn(T, W, device=DEV, dtype=torch.bfloat16)
    do = torch.randn(T, hq * D, device=DEV, dtype=torch.bfloat16)
    cos = torch.ones(S, D // 2, device=DEV)
    sin = torch.zeros(S, D // 2, device=DEV)
    buf, lse, dqkv = _raw(qkv, do, cos, sin, hq, hkv, B, S, causal=causal)
    x = qkv.view(B, S, hq + 2 * hkv, D)
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv], x[:, :, hq + hkv:]
    o, lse_p = C.attn_fwd(q, k, v, None, sc, causal, None)
    dq, dk, dv = C.attn_bwd(do.view(B, S, hq, D), q, k, v, o, lse_p, None, None, None, sc, causal, None)
    torch.cuda.synchronize()
    g = dqkv.view(B, S, hq + 2 * hkv, D)
    assert torch.equal(buf.view(B, S, hq, D), o), "o"
    assert torch.equal(lse, lse_p), "lse"
    assert torch.equal(g[:, :, :hq], dq), "dq"
    assert torch.equal(g[:, :, hq:hq + hkv], dk), "dk"
    assert torch.equal(g[:, :, hq + hkv:], dv), "dv"


# ------------------------------------------------------------------ 8. no fallback, model level
def test_llama_tiny_d64_packed_runs_on_the_kernels_only(monkeypatch):
    """tests/test_varlen.py::_check_model for llama-tiny-d64 with every slower path closed."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.ops import Varlen, _ref, fused
    lens, tol = [37, 64, 20, 129], 3e-2
    dev = torch.device(DEV, 0)

    def boom(*a, **k):
        raise AssertionError("head_dim 64 rope_attention left the qkv-native kernels")
    monkeypatch.setattr(fused, "flash_attention", boom)
    monkeypatch.setattr(_ref, "attention", boom)
    monkeypatch.setattr(_ref, "apply_rope", boom)
    torch.manual_seed(0)
    m = build_llama("llama-tiny-d64", device=dev, dtype=torch.bfloat16, seed=3)
    assert m.config.head_dim == 64
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, m.config.vocab_size, (n,), generator=g).to(dev) for n in lens]
    vl = Varlen(lens, dev)
    packed = torch.cat(seqs).view(1, -1)
    out = m(packed, labels=packed, varlen=vl, return_logits=True)
    ref_logits = torch.cat([m(s.view(1, -1), return_logits=True)["logits"][0] for s in seqs])
    err = (out["logits"][0].float() - ref_logits.float()).abs().max().item()
    assert err < tol, f"packed logits differ by {err}"
    losses = [m(s.view(1, -1), labels=s.view(1, -1))["loss"] for s in seqs]
    n = [len(s) - 1 for s in seqs]
    ref = sum(l * k for l, k in zip(losses, n)) / sum(n)
    assert abs(out["loss"].item() - ref.item()) < tol * 5
    m.zero_grad()
    out["loss"].backward()
    g_packed = {k: p.grad.float().clone() for k, p in m.named_parameters()}
    m.zero_grad()
    ref2 = sum(m(s.view(1, -1), labels=s.view(1, -1))["loss"] * k for s, k in zip(seqs, n)) / sum(n)
    ref2.backward()
    for k, p in m.named_parameters():
        d = (g_packed[k] - p.grad.float()).norm() / p.grad.float().norm().clamp_min(1e-12)
        assert d < tol * 10, f"grad {k}: rel err {d.item():.3g}"


# ------------------------------------------------------------------ 9. the door
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2)])
def test_door_selects_the_old_path(hq, hkv, monkeypatch):
    from gke_ray_train_amd.ops import fused

    def boom(*a, **k):
        raise AssertionError("the qkv-native op ran with the door closed")
    monkeypatch.setattr(fused, "_ROPE_ATTN_D64", False)
    monkeypatch.setattr(fused._RopeAttentionD64, "apply", boom)
    _op_parity(hq, hkv)


# ------------------------------------------------------------------ 10. refusals
def test_bindings_refuse_what_the_kernels_do_not_handle():
    C = _C()
    hq, hkv, T = 4, 2, 96
    W = (hq + 2 * hkv) * D
    qkv = torch.randn(T, W, device=DEV, dtype=torch.bfloat16)
    o = torch.empty(T, hq, D, device=DEV, dtype=torch.bfloat16)
    cos = torch.ones(T, D // 2, device=DEV)
    sin = torch.zeros(T, D // 2, device=DEV)
    cu = torch.tensor([0, 40, T], dtype=torch.int32)
    sc = D ** -0.5
    with pytest.raises(RuntimeError, match="rope_attn_fwd_d64.*bf16"):
        C.rope_attn_fwd_d64(qkv.float(), cos, sin, o, 1, T, hq, hkv, sc, True)
    with pytest.raises(RuntimeError, match=r"rope_attn_fwd_d64.*\(Hq \+ 2 Hkv\) \* 64"):
        C.rope_attn_fwd_d64(qkv[:, :W - D].contiguous(), cos, sin, o, 1, T, hq, hkv, sc, True)
    with pytest.raises(RuntimeError, match="rope_attn_fwd_d64.*cos/sin tables"):
        C.rope_attn_fwd_d64(qkv, cos[:55], sin[:55], o, 1, T, hq, hkv, sc, True, cu_seqlens=cu.to(DEV), max_seqlen=56)
    with pytest.raises(RuntimeError, match="rope_attn_fwd_d64.*cos/sin tables"):
        C.rope_attn_fwd_d64(qkv, cos[:T - 1], sin[:T - 1], o, 1, T, hq, hkv, sc, True)
    with pytest.raises(RuntimeError, match="rope_attn_fwd_d64.*cu_seqlens.*device"):
        C.rope_attn_fwd_d64(qkv, cos, sin, o, 1, T, hq, hkv, sc, True, cu_seqlens=cu, max_seqlen=56)
    with pytest.raises(RuntimeError, match="rope_attn_fwd_d64.*contiguous"):
        C.rope_attn_fwd_d64(torch.randn(T, 2 * W, device=DEV, dtype=torch.bfloat16)[:, :W], cos, sin, o, 1, T, hq, hkv,
                            sc, True)
    lse = C.rope_attn_fwd_d64(qkv, cos, sin, o, 1, T, hq, hkv, sc, True, cu_seqlens=cu.to(DEV), max_seqlen=56)
    assert lse.shape == (2, hq, 56)
    with pytest.raises(RuntimeError, match="rope_attn_bwd_d64.*dqkv"):
        C.rope_attn_bwd_d64(torch.randn_like(o), qkv, cos, sin, o, lse, torch.empty(T, W, device=DEV), 1, T, hq, hkv,
                            sc, True, cu_seqlens=cu.to(DEV), max_seqlen=56)
    torch.cuda.synchronize()
