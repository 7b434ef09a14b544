"""Decode at head_dim 64 (Llama-3.2-1B geometry): the split-K decode attention kernel
(decode_attention.hip at D = 64), the qkv GEMV's RoPE + KV-append epilogue at D = 64 (gemv.hip) and
their wiring into ``ops.flash_attention``, ``GraphDecoder`` and ``generate()``.

References are the fp32 math of ``ops/_ref.py``. The attention tolerance is
``test_kernels_gpu.py::test_decode_attention``'s (1e-2 absolute and relative), the GEMV epilogue's
is ``test_gemv_rope_epilogue``'s (1e-2) and the decoder logits' is
``test_decode_fused_norm_matches_unfused``'s (2e-2).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
QNAN = 0x7FC00000


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _close(a, b, atol, rtol, what=""):
    """The comparison of test_kernels_gpu.py (whose tolerances the tests here take over): under
    0.1 % of the elements past atol + rtol |ref|, and none past 10x that."""
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.4g}, worst element at {worst:.3f}x its tolerance")
    assert not torch.isnan(a).any(), f"{what}: NaN in kernel output"
    assert (err > tol).float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"


class _Counting:
    """Proxy of the extension module that counts the calls of every function by name; a
    ``gemv_fused`` call with the RoPE epilogue (``cos=``) also counts as ``gemv_fused:rope``."""

    def __init__(self, C):
        self._C, self.calls = C, {}

    def __getattr__(self, name):
        fn = getattr(self._C, name)
        if not callable(fn) or name.isupper():
            return fn
        calls = self.calls

        def call(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            if name == "gemv_fused" and k.get("cos") is not None:
                calls["gemv_fused:rope"] = calls.get("gemv_fused:rope", 0) + 1
            return fn(*a, **k)
        return call


@pytest.fixture
def counting(monkeypatch):
    from gke_ray_train_amd import _native
    proxy = _Counting(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: proxy)
    return proxy


def _qkv(B, Sk, hq, hkv, seed, d=D):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, 1, hq, d, device=DEV, dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, Sk, hkv, d, device=DEV, dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, Sk, hkv, d, device=DEV, dtype=torch.bfloat16, generator=g)
    return q, k, v


# ------------------------------------------------------------------ 1. kernel vs fp32 math
@pytest.mark.parametrize("B,Sk,hq,hkv,lens", [
    (1, 1, 4, 4, None),                 # a single key
    (1, 31, 8, 4, None),                # the 32-key workgroup step: one short, exact, one over
    (1, 32, 8, 4, None),
    (1, 33, 8, 4, None),
    (3, 97, 4, 2, [97, 40, 1]),         # valid lengths on the one-launch path (Sk <= 256: one split)
    (1, 256, 8, 4, None),               # the last Sk on the one-launch path, and the first with
    (1, 257, 8, 4, None),               # split + combine (9 splits of 32 keys)
    (3, 290, 4, 2, [290, 40, 1]),       # 10 splits of 32 keys; rows 1 and 2 leave splits empty
    (1, 600, 32, 8, None),              # G = 4, the Llama-3.2-1B geometry, 19 splits
    (2, 1300, 16, 2, [1300, 517]),      # G = 8 with valid lengths
    (2, 2100, 2, 2, None),              # G = 1, split count at its cap of 64 (ceil(2100 / 32) = 66)
])
def test_decode_attention_d64_matches_fp32_math(counting, B, Sk, hq, hkv, lens):
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import _ref
    q, k, v = _qkv(B, Sk, hq, hkv, B * Sk + hq)
    sl = torch.tensor(lens, device=DEV, dtype=torch.int32) if lens else None
    with torch.no_grad():
        o = ops.flash_attention(q, k, v, causal=sl is None, seqlens_k=sl)
    assert counting.calls.get("attn_decode_d64", 0) == 1 and "attn_fwd" not in counting.calls, counting.calls
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    ref = _ref.attention(q.float(), k.float(), v.float(), causal=sl is None, seqlens_k=sl)
    _close(o, ref, 1e-2, 1e-2, "decode attention d64")


# ------------------------------------------------------------------ 2. strided cache view
@pytest.mark.parametrize("B,L,n,hq,hkv", [(2, 96, 45, 4, 2), (1, 600, 290, 32, 8)])
def test_cache_slice_and_full_cache_with_seqlens_agree(B, L, n, hq, hkv):
    """k / v as ``cache[:, :n]`` views of a longer cache == the full cache with ``seqlens_k = n``
    (the graph decoder's call), bitwise; rows past n are NaN, so a read past the valid length shows.
    Both calls of a pair partition the keys alike, so the partial sums combine in the same order:
    (96, 45) is one split in both calls (Sk <= 256), (600, 290) is 32 keys per split in both (10
    resp. 19 splits; the longer call only adds empty ones). A pair that straddles the one-launch
    threshold agrees within tolerance only."""
    from gke_ray_train_amd.ops import _ref
    C = _C()
    g = torch.Generator(device=DEV).manual_seed(L + n)
    q = torch.randn(B, 1, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc = torch.randn(B, L, hkv, D, device=DEV, dtype=torch.bfloat16, generator=g)
    vc = torch.randn(B, L, hkv, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc[:, n:] = float("nan")
    vc[:, n:] = float("nan")
    kv, vv = kc[:, :n], vc[:, :n]
    assert not kv.is_contiguous() or B == 1
    a = C.attn_decode_d64(q, kv, vv, None, D ** -0.5)
    b = C.attn_decode_d64(q, kc, vc, torch.full((B,), n, device=DEV, dtype=torch.int32), D ** -0.5)
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert torch.equal(a, b)
    ref = _ref.attention(q.float(), kv.float(), vv.float(), causal=True)
    _close(a, ref, 1e-2, 1e-2, "cache slice")
    _close(b, ref, 1e-2, 1e-2, "full cache + seqlens_k")


def test_split_partials_contract():
    """The per-split partial states: with q = 0 every score is 0, so a split's max is 0 and its sum
    is its key count, read here directly. Sk = 300 gives 10 splits; every split takes a multiple of
    the 32-key workgroup step (row 0: nine of 32 and one of 12; row 1 with 70 valid keys: 32, 32, 6
    and seven empty ones), an empty split emits max = -inf, sum = 0 and a zero output, and a
    non-empty split's output is the fp32 sum of its V rows (exp2(0) = 1: the only rounding is the
    fp32 summation order, far inside 1e-4)."""
    C = _C()
    B, Sk, hq, hkv = 2, 300, 4, 2
    _, k, v = _qkv(B, Sk, hq, hkv, 3)
    q = torch.zeros(B, 1, hq, D, device=DEV, dtype=torch.bfloat16)
    lens = [300, 70]
    sl = torch.tensor(lens, device=DEV, dtype=torch.int32)
    o, part_o, part_m, part_l = C.attn_decode_d64_partials(q, k, v, sl, D ** -0.5)
    assert part_l.shape == (B, hq, 10) and part_m.shape == (B, hq, 10) and part_o.shape == (B, hq, 10, D)
    for b, n in enumerate(lens):
        counts = [max(0, min(32, n - 32 * s)) for s in range(10)]
        want = torch.tensor(counts, device=DEV, dtype=torch.float32).expand(hq, 10)
        print(f"row {b}: split sums {part_l[b, 0].tolist()}")
        torch.testing.assert_close(part_l[b], want, rtol=0, atol=1e-4)
        empty = want == 0
        assert (part_m[b][empty] == float("-inf")).all() and (part_m[b][~empty] == 0).all()
        vs = torch.zeros(10, hkv, D, device=DEV)
        for s, c in enumerate(counts):
            vs[s] = v[b, 32 * s:32 * s + c].float().sum(0)
        want_o = vs.transpose(0, 1).repeat_interleave(hq // hkv, dim=0)  # [hq, 10, D]
        torch.testing.assert_close(part_o[b], want_o, rtol=1e-4, atol=1e-4)
    ref = torch.stack([v[b, :n].float().mean(0) for b, n in enumerate(lens)])  # uniform softmax
    _close(o[:, 0], ref.repeat_interleave(hq // hkv, dim=1), 1e-2, 1e-2, "uniform attention")


# ------------------------------------------------------------------ 3. stale LDS
@pytest.mark.parametrize("Sk", [200, 333])  # one launch; split + combine
def test_decode_attention_d64_reads_no_stale_lds(Sk):
    C = _C()
    q, k, v = _qkv(2, Sk, 8, 2, 7)
    sl = torch.tensor([Sk, 90], device=DEV, dtype=torch.int32)
    dev = torch.cuda.current_device()
    outs = []
    for pattern in (QNAN, 0):
        C.lds_fill(pattern, dev)
        outs.append(C.attn_decode_d64(q, k, v, sl, D ** -0.5))
    assert torch.isfinite(outs[0].float()).all() and torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(C.attn_decode_d64(q, k, v, sl, D ** -0.5), C.attn_decode_d64(q, k, v, sl, D ** -0.5))


# ------------------------------------------------------------------ 4. refusals
def test_attn_decode_d64_refusals():
    """Every refused call's operands lie inside live allocations."""
    C = _C()
    sc = D ** -0.5
    q, k, v = _qkv(2, 16, 4, 2, 1)
    o = C.attn_decode_d64(q, k, v, None, sc)  # the accepted baseline
    assert o.shape == q.shape
    q128, k128, v128 = _qkv(2, 16, 4, 2, 2, d=128)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        C.attn_decode_d64(q128, k128, v128, None, sc)
    q2 = torch.randn(2, 2, 4, D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="one query token"):
        C.attn_decode_d64(q2, k, v, None, sc)
    with pytest.raises(RuntimeError, match="bf16"):
        C.attn_decode_d64(q.float(), k.float(), v.float(), None, sc)
    q6 = torch.randn(2, 1, 6, D, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GQA group"):
        C.attn_decode_d64(q6, k, v, None, sc)
    # head stride 68 elements (136 bytes): the 16-byte loads of head 1 would be misaligned
    wide = torch.randn(2, 16, 2, D + 4, device=DEV, dtype=torch.bfloat16)
    ks = wide[..., :D]
    assert ks.shape == k.shape and ks.stride(3) == 1 and ks.stride(2) % 8 != 0
    with pytest.raises(RuntimeError, match="stride|alignment"):
        C.attn_decode_d64(q, ks, v, None, sc)
    with pytest.raises(RuntimeError, match="stride|alignment"):
        C.attn_decode_d64(q, k, ks, None, sc)
    with pytest.raises(RuntimeError, match="seqlens_k"):
        C.attn_decode_d64(q, k, v, torch.tensor([16, 3], device=DEV, dtype=torch.int64), sc)
    with pytest.raises(RuntimeError, match="seqlens_k"):
        C.attn_decode_d64(q, k, v, torch.tensor([16, 3, 2], device=DEV, dtype=torch.int32), sc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. GEMV RoPE epilogue
@pytest.mark.parametrize("hd,M,hq,hkv,normx", [(64, 1, 32, 8, True), (64, 2, 8, 8, False), (64, 4, 4, 1, True),
                                               (128, 2, 4, 2, True)])
def test_gemv_rope_epilogue_d64(hd, M, hq, hkv, normx):
    """qkv GEMV with the RoPE + KV-cache append epilogue at head_dim 64 (and one head_dim-128 case
    through the same templated code) == GEMV + rope_append: q and the k cache within 1e-2 (same bf16
    qkv, the rotation's fp32 contraction may differ by an ulp), the v cache bitwise, only the slot
    at pos[m] changed; a position past the cache writes nothing. The RoPE table has twice the
    cache's rows, so positions past the cache are still valid table rows."""
    C, L = _C(), 16
    g = torch.Generator(device=DEV).manual_seed(M * hq + hkv + hd)
    K = 512
    N = (hq + 2 * hkv) * hd
    h = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16, generator=g) * 0.05
    nw = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(torch.bfloat16)
    acc = torch.zeros(2, M, 64, dtype=torch.int64, device=DEV)
    acc[1, :, 0] = torch.round(h.double().pow(2).sum(-1) * 2 ** 20).long()
    ang = torch.arange(2 * L, device=DEV, dtype=torch.float32)[:, None] * torch.rand(hd // 2, device=DEV, generator=g)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    pos = torch.tensor([3, 11, 0, 15][:M], device=DEV, dtype=torch.int32)
    if M == 2 and hq == 8:
        pos[1] = L + 5  # one position past the cache: no write for that row
    kc0 = torch.randn(M, L, hkv, hd, device=DEV, dtype=torch.bfloat16, generator=g)
    vc0 = torch.randn(M, L, hkv, hd, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, vc, kr, vr = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    if normx:
        q = C.gemv_fused(h, w, acc, 1, g=nw, eps=1e-5, cos=cos, sin=sin, pos=pos, kc=kc, vc=vc, hq=hq, hkv=hkv)
        qkv = C.gemv_fused(h, w, acc, 1, g=nw, eps=1e-5)
    else:
        q = C.gemv_fused(h, w, acc, 1, cos=cos, sin=sin, pos=pos, kc=kc, vc=vc, hq=hq, hkv=hkv)
        qkv = C.gemv(h, w)
    assert q.shape == (M, hq, hd)
    qr = C.rope_append(qkv, cos, sin, pos, hq, hkv, hd, cos.shape[0], kr, vr, 1)
    ok = (pos < L).tolist()
    for m in range(M):
        if ok[m]:
            _close(q[m], qr[m].view(hq, hd), 1e-2, 1e-2, f"rope epilogue q row {m}")
    _close(kc, kr, 1e-2, 1e-2, "rope epilogue k cache")
    assert torch.equal(vc, vr)
    assert not torch.equal(kc, kc0) and not torch.equal(vc, vc0)
    for m in range(M):  # only the slot at pos[m] changed, and all of it did
        keep = torch.ones(L, dtype=torch.bool)
        if ok[m]:
            p = int(pos[m])
            keep[p] = False
            assert (kc[m, p] != kc0[m, p]).float().mean() > 0.9 and (vc[m, p] != vc0[m, p]).float().mean() > 0.9
        assert torch.equal(kc[m, keep], kc0[m, keep]) and torch.equal(vc[m, keep], vc0[m, keep])


def test_gemv_rope_epilogue_refuses_other_head_dims():
    C = _C()
    M, K, hq, hkv, L = 1, 64, 2, 1, 4
    h = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    acc = torch.zeros(2, M, 64, dtype=torch.int64, device=DEV)
    pos = torch.zeros(M, device=DEV, dtype=torch.int32)
    for hd, tab in ((96, 48), (64, 64)):  # a 96-wide head; a 128-wide table for 64-wide heads
        w = torch.randn((hq + 2 * hkv) * hd, K, device=DEV, dtype=torch.bfloat16)
        kc = torch.zeros(M, L, hkv, hd, device=DEV, dtype=torch.bfloat16)
        cos = torch.ones(L, tab, device=DEV)
        with pytest.raises(RuntimeError, match="head_dim"):
            C.gemv_fused(h, w, acc, 1, cos=cos, sin=torch.zeros_like(cos), pos=pos, kc=kc, vc=kc.clone(),
                         hq=hq, hkv=hkv)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. graph decoder
LOGIT_TOL = 2e-2  # absolute and relative, test_decode_fused_norm_matches_unfused
SEED = 95


@pytest.mark.parametrize("B", [1, 2])
def test_graph_decoder_d64_matches_eager(counting, B):
    """llama-tiny-d64: fused-norm graph decoder, unfused graph decoder and eager ``forward_cached``
    give the same logits. All three are teacher-forced with the eager path's greedy tokens, so one
    near-tie cannot derail the later steps; the argmax must agree wherever the eager top-1 / top-2
    margin exceeds twice the logit tolerance, and at least half the steps must be that decisive."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    steps = 6
    # seed 95 (model and prompt): a random-init model's logits are nearly flat, and of seeds 0-119
    # this one has the most decisive eager steps (6 of 6 at B = 1, 11 of 12 at B = 2, read off the
    # eager path alone); many seeds have fewer than half
    m = build_llama("llama-tiny-d64", device=DEV, dtype=torch.bfloat16, seed=SEED).eval()
    assert m.config.head_dim == 64
    torch.manual_seed(SEED)
    ids = torch.randint(0, m.config.vocab_size, (B, 12), device=DEV)
    cache = G.KVCache(m.config, B, 32, DEV, torch.bfloat16)
    eager = [G.forward_cached(m, ids, cache)]
    toks = [eager[0].argmax(-1)]
    for _ in range(steps):
        eager.append(G.forward_cached(m, toks[-1][:, None], cache))
        toks.append(eager[-1].argmax(-1))
    eager = torch.stack(eager[1:])  # [steps, B, V]: the one-token steps
    outs = {}
    for name, fused in (("fused", True), ("unfused", False)):
        counting.calls.clear()
        G._GEMV_NORM = fused
        try:
            dec = G.GraphDecoder(m, B, 32)
            assert (dec.norm_ws is not None) == fused
            dec.prefill(ids)
            outs[name] = torch.stack([dec.step(toks[t]).clone() for t in range(steps)])
        finally:
            G._GEMV_NORM = True
        assert counting.calls.get("attn_decode_d64", 0) > 0, counting.calls
        assert (counting.calls.get("gemv_fused:rope", 0) > 0) == fused, counting.calls
    top2 = eager.topk(2, -1).values
    margin = top2[..., 0] - top2[..., 1]
    decisive = margin > 2 * (LOGIT_TOL + LOGIT_TOL * top2[..., 0].abs())
    print(f"decisive steps: {int(decisive.sum())} of {decisive.numel()}, margins {margin.flatten().tolist()}")
    for name, lg in outs.items():
        err = (lg - eager).abs()
        print(f"{name} vs eager: max err {err.max().item():.4g}, argmax agrees at "
              f"{int((lg.argmax(-1) == eager.argmax(-1)).sum())} of {decisive.numel()} steps")
    assert decisive.float().mean().item() >= 0.5, "pick a seed with decisive greedy steps"
    for name, lg in outs.items():
        _close(lg, eager, LOGIT_TOL, LOGIT_TOL, f"{name} graph decoder vs eager logits")
        assert torch.equal(lg.argmax(-1)[decisive], eager.argmax(-1)[decisive]), name
    _close(outs["fused"], outs["unfused"], LOGIT_TOL, LOGIT_TOL, "fused vs unfused graph decoder logits")


# ------------------------------------------------------------------ 7. generate() end to end
def test_generate_d64_takes_the_graph_decoder(monkeypatch):
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    made = []

    class Counted(G.GraphDecoder):
        def __init__(self, *a, **k):
            made.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(G, "GraphDecoder", Counted)
    torch.manual_seed(0)
    m = build_llama("llama-tiny-d64", device=DEV, dtype=torch.bfloat16, seed=0).eval()
    B, S = 2, 12
    ids = torch.randint(0, m.config.vocab_size, (B, S), device=DEV)
    out = m.generate(ids, max_new_tokens=16)
    assert len(made) == 1
    assert out.shape == (B, S + 16) and torch.equal(out[:, :S], ids)
    out_eager = m.generate(ids, max_new_tokens=16, use_graph=False)
    assert len(made) == 1, "use_graph=False must not construct a GraphDecoder"
    assert out_eager.shape == (B, S + 16)
    # the cache-overflow refusals still raise
    dec = G.GraphDecoder(m, B, S + 1)
    nxt = dec.prefill(ids).argmax(-1)
    dec.step(nxt)
    assert dec.cache.len == S + 1
    with pytest.raises(RuntimeError, match="KV cache full"):
        dec.step(nxt)
    cache = G.KVCache(m.config, B, S, DEV, torch.bfloat16)
    G.forward_cached(m, ids, cache)
    with pytest.raises(ValueError, match="KV cache overflow"):
        G.forward_cached(m, ids[:, :1], cache)
