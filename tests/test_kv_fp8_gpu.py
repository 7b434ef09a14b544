"""fp8 KV cache on the GPU: the quantising append and the dequantiser (kv_fp8.hip) against the host
definition of the format (``ops/_ref.py::kv_fp8_*``), the split-K decode kernel reading e4m3fn codes
(decode_attention.hip, ``ops.decode_attention_fp8``) against fp32 math on the dequantised cache, and
``generate(kv_cache_dtype="fp8")`` / ``GraphDecoder`` on the two tiny models of the decode tests.

Comparison rule and tolerances are test_decode_d64_gpu.py's: ``_close`` (under 0.1 % of the elements
past atol + rtol |ref|, none past 10x), 1e-2 / 1e-2 for the attention kernel (the bf16 kernel's,
whose fp32 FMA chain it shares; the reference sees the same quantised values), 2e-2 / 2e-2 between
decode paths. The format's own bound per element is |dequant - x| <= max(|x| 2^-4, scale 2^-10)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child process starts from this file, not from pytest
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOGIT_TOL = 2e-2
MODELS = ["llama-tiny-gqa", "llama-tiny-d64"]   # head_dim 128 and 64
SENT_CODE, SENT_SCALE = 0x55, -7.0
_cache = {}


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _ref():
    from gke_ray_train_amd.ops import _ref
    return _ref


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _close(a, b, atol, rtol, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.4g}, worst element at {worst:.3f}x its tolerance")
    assert not torch.isnan(a).any(), f"{what}: NaN in kernel output"
    assert (err > tol).float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"
    return err.max().item()


def fp8_bound(x, scale):
    return torch.maximum(x.float().abs() * 2.0 ** -4, scale.unsqueeze(-1) * 2.0 ** -10)


def tie_values():
    """Every finite code's value, every midpoint between neighbouring codes (exact in bf16) and each
    midpoint +- one bf16 ulp, both signs (the vectors of test_kv_fp8_cpu.py)."""
    tab = _ref().kv_fp8_table()
    pos = tab[:127]
    mb = ((pos[:-1] + pos[1:]) / 2).bfloat16()
    up = (mb.view(torch.int16) + 1).view(torch.bfloat16)
    dn = (mb.view(torch.int16) - 1).view(torch.bfloat16)
    vals = torch.cat([pos.bfloat16(), mb, up, dn])
    return torch.cat([vals, -vals])


def quantize_host(x):
    """``_ref.kv_fp8_quantize`` on the host (torch's CPU e4m3fn cast is the reference), back on x's device."""
    codes, scale = _ref().kv_fp8_quantize(x.cpu())
    return codes.to(x.device), scale.to(x.device)


# ------------------------------------------------------------------ 1. rope_append_fp8
def _positions(M, tpr, L, S, g):
    """One position per token, distinct inside a row: seeded random slots below L - 1, then the edge
    cases over the first tokens (-1 and L are outside the cache, L - 1 its last slot) and S, the
    first position outside the rope table, over the last."""
    B = M // tpr
    pos = torch.rand(B, L - 1, device=DEV, generator=g).argsort(1)[:, :tpr].flatten().int()
    if M >= 3:
        pos[0], pos[1], pos[M - 1] = -1, L - 1, L
    if M >= 4:
        pos[M - 2] = S
    if L > S and M >= 5:   # inside the cache, outside the rope table: only the p < S predicate skips it
        pos[2] = S + (L - S) // 2
    return pos


APPEND_CASES = [(D, hq, hkv, M, tpr)
                for D in (64, 128) for hq, hkv in ((4, 4), (8, 2), (32, 8))
                for M, tpr in ((1, 1), (3, 1), (3, 3), (70, 1), (70, 7))]
# the launch is capped at 2048 workgroups of 256 lanes, D / 16 lanes per head: 1400 tokens of 48
# heads at head_dim 128 are 537,600 work items, the smallest round count past one grid pass
APPEND_CASES.append((128, 32, 8, 1400, 1))
# a cache longer than the rope table (L = 48 > S = 40): a position in [S, L) must be skipped too
LONG_CACHE = {(64, 8, 2, 9, 1), (128, 8, 2, 9, 3)}
APPEND_CASES += sorted(LONG_CACHE)


@pytest.mark.parametrize("D,hq,hkv,M,tpr", APPEND_CASES)
def test_rope_append_fp8_matches_ref(D, hq, hkv, M, tpr):
    ref, C = _ref(), _C()
    g = _gen(D + hq + M + tpr)
    B, L, S = M // tpr, 48 if (D, hq, hkv, M, tpr) in LONG_CACHE else 24, 40
    heads = hq + 2 * hkv
    qkv = torch.randn(M, heads * D, device=DEV, dtype=torch.bfloat16, generator=g)
    # V heads of the first tokens: the tie / subnormal vectors, each with a 448 so its scale is 1
    tv = tie_values().to(DEV)
    n_tie = min(M * hkv, -(-len(tv) // (D - 1)))     # vector i is V head i % hkv of token i // hkv
    flat = torch.zeros(n_tie * (D - 1), device=DEV, dtype=torch.bfloat16)
    flat[:min(len(tv), len(flat))] = tv[:len(flat)]
    i = torch.arange(n_tie, device=DEV)
    qkv.view(M, heads, D)[i // hkv, hq + hkv + i % hkv] = torch.cat(
        [torch.full((n_tie, 1), 448.0, device=DEV, dtype=torch.bfloat16), flat.view(n_tie, D - 1)], 1)
    cos, sin = ref.rope_tables(S, D, device=DEV)
    pos = _positions(M, tpr, L, S, g)
    ok = (pos >= 0) & (pos < L) & (pos < S)
    assert L <= S or bool(((pos >= S) & (pos < L)).any())

    def caches():
        return (torch.full((B, L, hkv, D), SENT_CODE, device=DEV, dtype=torch.uint8),
                torch.full((B, L, hkv), SENT_SCALE, device=DEV))
    (kc, ksc), (vc, vsc) = caches(), caches()
    k_out = torch.full((M, hkv, D), 3.0, device=DEV, dtype=torch.bfloat16)
    q = C.rope_append_fp8(qkv, cos, sin, pos, hq, hkv, D, S, kc, vc, ksc, vsc, tpr, k_out=k_out)
    # the bf16 kernel on the same input: the q it returns and the K rows its cache holds
    kb = torch.zeros(B, L, hkv, D, device=DEV, dtype=torch.bfloat16)
    vb = torch.zeros_like(kb)
    qb = C.rope_append(qkv, cos, sin, pos, hq, hkv, D, S, kb, vb, tpr)
    torch.cuda.synchronize()
    rows = torch.arange(M, device=DEV) // tpr
    slot = pos.long().clamp(0, L - 1)
    assert torch.equal(q[ok], qb[ok])
    k_ref = kb[rows, slot]                       # [M, hkv, D], meaningful where ok
    assert torch.equal(k_out[ok], k_ref[ok])
    assert (k_out[~ok] == 3.0).all()             # a skipped token writes nothing at all
    # V: codes and scales bit-exact
    want_vc, want_vs = quantize_host(qkv.view(M, heads, D)[:, hq + hkv:])
    assert torch.equal(vc[rows, slot][ok], want_vc[ok])
    assert torch.equal(vsc[rows, slot][ok], want_vs[ok])
    assert (want_vs.flatten()[:n_tie] == 1.0).all()
    # K: bit-exact where RoPE is the identity (position 0), and everywhere against the quantised
    # image of the K the bf16 cache holds; its dequantised rows within the format's bound plus one
    # bf16 ulp (2^-7 |k|) of that K
    got_kc, got_ks = kc[rows, slot], ksc[rows, slot]
    want_kc, want_ks = quantize_host(k_ref)
    assert torch.equal(got_kc[ok], want_kc[ok]) and torch.equal(got_ks[ok], want_ks[ok])
    deq = ref.kv_fp8_dequantize(got_kc.cpu(), got_ks.cpu()).to(DEV)
    lim = fp8_bound(k_ref, got_ks) + k_ref.float().abs() * 2.0 ** -7
    assert ((deq - k_ref.float()).abs() <= lim)[ok].all()
    assert not ((got_kc[ok] & 0x7F) == 0x7F).any()
    # untouched slots keep the sentinel
    written = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    written[rows[ok], slot[ok]] = True
    for codes, scales in ((kc, ksc), (vc, vsc)):
        assert (codes[~written] == SENT_CODE).all() and (scales[~written] == SENT_SCALE).all()
    assert int(ok.sum()) == int(written.sum()) and (M < 3 or int((~ok).sum()) >= 2)


@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_fp8_k_is_bit_exact_at_position_zero(D):
    ref, C = _ref(), _C()
    hq, hkv, M = 8, 2, 6
    g = _gen(D)
    qkv = torch.randn(M, (hq + 2 * hkv) * D, device=DEV, dtype=torch.bfloat16, generator=g)
    tv = tie_values().to(DEV)
    k3 = qkv.view(M, hq + 2 * hkv, D)[:, hq:hq + hkv]
    k3[0, 0, 0], k3[0, 0, 1:] = 448.0, tv[127:127 + D - 1]     # midpoints: they must tie to even
    cos, sin = ref.rope_tables(16, D, device=DEV)
    kc = torch.zeros(M, 4, hkv, D, device=DEV, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    ksc, vsc = torch.zeros(M, 4, hkv, device=DEV), torch.zeros(M, 4, hkv, device=DEV)
    C.rope_append_fp8(qkv, cos, sin, torch.zeros(M, device=DEV, dtype=torch.int32), hq, hkv, D, 16, kc, vc, ksc, vsc, 1)
    want_c, want_s = quantize_host(k3)
    assert torch.equal(kc[:, 0], want_c) and torch.equal(ksc[:, 0], want_s)
    assert ksc[0, 0, 0] == 1.0


# ------------------------------------------------------------------ 2. kv_fp8_dequant
@pytest.mark.parametrize("D", [64, 128])
def test_kv_fp8_dequant_equals_ref_bitwise(D):
    ref, C = _ref(), _C()
    g = _gen(5 + D)
    B, L, n, H = 3, 40, 29, 2
    big = torch.randint(0, 254, (B, L, 2 * H, D), device=DEV, generator=g).to(torch.uint8)
    big = big + (big >= 127).to(torch.uint8)            # skip 0x7F: codes 0..126 and 128..254
    codes = big[:, :, ::2]                              # a strided view (head stride 2 D)
    scale = torch.rand(B, L, H, device=DEV, generator=g) * 0.02 + 1e-4
    out = C.kv_fp8_dequant(codes, scale, n)
    assert out.shape == (B, n, H, D) and out.dtype == torch.bfloat16
    want = ref.kv_fp8_dequantize(codes[:, :n], scale[:, :n], torch.bfloat16)
    assert torch.equal(out, want)


# ------------------------------------------------------------------ 3. attention over the codes
def _fp8_kv(B, L, hkv, D, g):
    """A random fp8 cache: codes, scales and its dequantised fp32 image."""
    out = []
    for _ in range(2):
        x = torch.randn(B, L, hkv, D, device=DEV, dtype=torch.bfloat16, generator=g)
        c, s = quantize_host(x)
        out += [c, s, _ref().kv_fp8_dequantize(c, s), x]
    return out  # kc, ks, kd, kx, vc, vs, vd, vx


def _attn_ref(q, kd, vd, lens, scale=None):
    """fp32 math per token: token t of T sees the row's keys [0, len - (T - 1 - t))."""
    B, T = q.shape[:2]
    lens = lens.long() if lens is not None else torch.full((B,), kd.shape[1], device=q.device)
    return torch.cat([_ref().attention(q[:, t:t + 1].float(), kd, vd, causal=False, scale=scale,
                                       seqlens_k=lens - (T - 1 - t)) for t in range(T)], 1)


D64_CASES = [(1, 1, 4, 4, None), (1, 31, 8, 4, None), (1, 32, 8, 4, None), (1, 33, 8, 4, None),
             (3, 97, 4, 2, [97, 40, 1]), (1, 256, 8, 4, None), (1, 257, 8, 4, None), (3, 290, 4, 2, [290, 40, 1]),
             (1, 600, 32, 8, None), (2, 1300, 16, 2, [1300, 517]), (2, 2100, 2, 2, None)]
D128_CASES = [(1, 1, 4, 4, None), (1, 15, 8, 4, None), (1, 16, 8, 4, None), (1, 17, 8, 4, None),
              (3, 97, 4, 2, [97, 40, 1]), (1, 600, 32, 8, None), (2, 1300, 16, 2, [1300, 517])]


@pytest.mark.parametrize("D,B,Sk,hq,hkv,lens", [(64, *c) for c in D64_CASES] + [(128, *c) for c in D128_CASES])
def test_decode_attention_fp8_matches_fp32_math(D, B, Sk, hq, hkv, lens):
    from gke_ray_train_amd import ops
    g = _gen(B * Sk + hq + D)
    q = torch.randn(B, 1, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, ks, kd, _, vc, vs, vd, _ = _fp8_kv(B, Sk, hkv, D, g)
    sl = torch.tensor(lens, device=DEV, dtype=torch.int32) if lens else None
    o = ops.decode_attention_fp8(q, kc, vc, ks, vs, seqlens_k=sl)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    _close(o, _attn_ref(q, kd, vd, sl), 1e-2, 1e-2, f"fp8 decode attention D={D}")


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_fp8_multi_token(D, G, T):
    """Sk = 70 is 3 (head_dim 64) or 5 (128) splits; row 1 leaves the last ones empty and row 2 has
    ``seqlens_k = T``: its first token sees one key."""
    from gke_ray_train_amd import ops
    g = _gen(D + 10 * G + T)
    B, Sk, hkv = 3, 70, 2
    q = torch.randn(B, T, hkv * G, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, ks, kd, _, vc, vs, vd, _ = _fp8_kv(B, Sk, hkv, D, g)
    sl = torch.tensor([70, 20, T], device=DEV, dtype=torch.int32)
    o = ops.decode_attention_fp8(q, kc, vc, ks, vs, seqlens_k=sl)
    _close(o, _attn_ref(q, kd, vd, sl), 1e-2, 1e-2, f"fp8 decode attention D={D} G={G} T={T}")


@pytest.mark.parametrize("D,L,n,hq,hkv", [(64, 96, 45, 4, 2), (64, 600, 290, 32, 8), (128, 600, 290, 32, 8)])
def test_fp8_slots_past_the_valid_length_are_never_read(D, L, n, hq, hkv):
    """Slots past n hold the NaN code and NaN scales; the full cache with ``seqlens_k = n`` equals the
    sliced views bitwise (both calls of a pair partition the keys alike, as in
    test_decode_d64_gpu.py::test_cache_slice_and_full_cache_with_seqlens_agree)."""
    from gke_ray_train_amd import ops
    B = 2 if L == 96 else 1
    g = _gen(L + n + D)
    q = torch.randn(B, 1, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, ks, kd, _, vc, vs, vd, _ = _fp8_kv(B, L, hkv, D, g)
    for c, s in ((kc, ks), (vc, vs)):
        c[:, n:] = 0x7F
        s[:, n:] = float("nan")
    a = ops.decode_attention_fp8(q, kc[:, :n], vc[:, :n], ks[:, :n], vs[:, :n])
    b = ops.decode_attention_fp8(q, kc, vc, ks, vs, seqlens_k=torch.full((B,), n, device=DEV, dtype=torch.int32))
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert torch.equal(a, b)
    _close(a, _attn_ref(q, kd[:, :n], vd[:, :n], None), 1e-2, 1e-2, "sliced fp8 cache")


def test_binding_refusals():
    from gke_ray_train_amd import ops
    C = _C()
    g = _gen(1)
    B, L, hq, hkv, D = 1, 32, 4, 2, 64
    q = torch.randn(B, 1, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, ks, _, kx, vc, vs, _, _ = _fp8_kv(B, L, hkv, D, g)
    sc = D ** -0.5
    C.attn_decode_fp8_d64(q, kc, vc, ks, vs, None, sc)
    with pytest.raises(RuntimeError, match="uint8 codes"):
        C.attn_decode_fp8_d64(q, kx, vc, ks, vs, None, sc)                  # bf16 K
    with pytest.raises(RuntimeError, match="bf16"):
        C.attn_decode_fp8_d64(q.float(), kc, vc, ks, vs, None, sc)          # fp32 q
    with pytest.raises(RuntimeError, match=r"fp32 \[B, L, Hkv\]"):
        C.attn_decode_fp8_d64(q, kc, vc, ks.bfloat16(), vs, None, sc)       # bf16 scales
    with pytest.raises(RuntimeError, match=r"fp32 \[B, L, Hkv\]"):
        C.attn_decode_fp8_d64(q, kc, vc, ks[:, :, :1], vs, None, sc)        # wrong scale shape
    wide = torch.zeros(B, L, hkv, D + 4, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        C.attn_decode_fp8_d64(q, wide[..., :D], vc, ks, vs, None, sc)       # head stride 68: misaligned
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        C.attn_decode_fp8_d64(q, wide.view(-1)[4:4 + kc.numel()].view(kc.shape), vc, ks, vs, None, sc)  # base + 4
    q3 = torch.randn(B, 1, 6, D, device=DEV, dtype=torch.bfloat16, generator=g)
    with pytest.raises(RuntimeError, match="GQA group"):
        C.attn_decode_fp8_d64(q3, kc, vc, ks, vs, None, sc)                 # G = 3
    q5 = torch.randn(B, 5, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    with pytest.raises(RuntimeError, match="1 to 4 query tokens"):
        C.attn_decode_fp8_d64(q5, kc, vc, ks, vs, None, sc)                 # T = 5
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_decode_fp8(q, kc, vc, ks, vs, None, sc)                      # the head_dim-128 binding
    q96 = torch.randn(B, 1, hq, 96, device=DEV, dtype=torch.bfloat16, generator=g)
    c96 = torch.zeros(B, L, hkv, 96, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="head_dim 96"):
        ops.decode_attention_fp8(q96, c96, c96, ks, vs)


# ------------------------------------------------------------------ 4. quantisation quality
@pytest.mark.parametrize("D", [64, 128])
def test_quantisation_error_of_the_attention_output(D):
    """The worst element difference, in float64 on the host, between attention over the exact K / V
    and over their quantise-dequantise images is the reference's own figure, known before the
    kernel runs; the kernel's output from the quantised cache is within that figure plus its
    1e-2 / 1e-2 tolerance of the exact attention."""
    from gke_ray_train_amd import ops
    g = _gen(D)
    B, Sk, hq, hkv = 1, 600, 32, 8
    q = torch.randn(B, 1, hq, D, device=DEV, dtype=torch.bfloat16, generator=g)
    kc, ks, kd, kx, vc, vs, vd, vx = _fp8_kv(B, Sk, hkv, D, g)

    def attn64(k, v):
        qh = q[0, 0].double().cpu() * D ** -0.5
        kk = k[0].double().cpu().repeat_interleave(hq // hkv, 1)            # [Sk, hq, D]
        vv = v[0].double().cpu().repeat_interleave(hq // hkv, 1)
        p = torch.softmax(torch.einsum("hd,shd->hs", qh, kk), -1)
        return torch.einsum("hs,shd->hd", p, vv)
    exact, quant = attn64(kx, vx), attn64(kd, vd)
    figure = (exact - quant).abs().max().item()
    o = ops.decode_attention_fp8(q, kc, vc, ks, vs)[0, 0].double().cpu()
    err = (o - exact).abs()
    print(f"D={D}: quantisation figure {figure:.4g}, kernel vs exact attention max err {err.max().item():.4g}")
    assert (err <= figure + 1e-2 + 1e-2 * exact.abs()).all()


# ------------------------------------------------------------------ 5. end to end
def _model(name, seed=0):
    from gke_ray_train_amd.models import build_llama
    if (name, seed) not in _cache:
        _cache[name, seed] = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=seed).eval()
    return _cache[name, seed]


def _ids(m, B, S, seed):
    return torch.randint(0, m.config.vocab_size, (B, S), device=DEV, generator=_gen(seed))


@pytest.mark.parametrize("name", MODELS)
def test_prefill_logits_equal_the_bf16_cache(name):
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    for B, S, mask in ((1, 12, None), (2, 9, torch.tensor([[1] * 9, [0] * 5 + [1] * 4], device=DEV))):
        ids = _ids(m, B, S, 3)
        a = G.forward_cached(m, ids, G.KVCache(m.config, B, 32, DEV, torch.bfloat16), mask)
        c = G.KVCache(m.config, B, 32, DEV, "fp8")
        b = G.forward_cached(m, ids, c, mask)
        assert torch.equal(a, b)
        assert c.k[0].dtype == torch.uint8 and c.k_scale[0].dtype == torch.float32 and bool(c.k_scale[0][0, 0].ne(0).all())


def graph_vs_eager(name, kv, seed=0, steps=8, B=1):
    """Max |graph step logits - eager step logits| over ``steps`` teacher-forced steps."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name, seed)
    ids = _ids(m, B, 12, seed)
    cache = G.KVCache(m.config, B, 32, DEV, "fp8" if kv else torch.bfloat16)
    lg = G.forward_cached(m, ids, cache)
    toks, eager = [], []
    for _ in range(steps):
        toks.append(lg.argmax(-1))
        lg = G.forward_cached(m, toks[-1][:, None], cache)
        eager.append(lg)
    dec = G.GraphDecoder(m, B, 32, kv_cache_dtype=kv)
    assert dec.cache.fp8 == bool(kv)
    dec.prefill(ids)
    graph = torch.stack([dec.step(t).clone() for t in toks])
    return graph, torch.stack(eager)


@pytest.mark.parametrize("name", MODELS)
def test_graph_step_logits_match_the_eager_step(name):
    """Graph step (norm-fused at B = 1: qkv GEMV, then ``rope_append_fp8``) against the
    ``use_graph=False`` step, 8 steps fed the same tokens, at the 2e-2 bound between decode paths;
    the bf16 cache's same comparison runs beside it. Measured max |difference| over model seeds
    0 / 1 / 2 (profiles/kv_fp8.md): head_dim 128 bf16 0 / 0 / 0, fp8 0 / 0.00781 / 0; head_dim 64 bf16
    0.00586 / 0.00781 / 0, fp8 0 / 0.00781 / 0.00391. All inside 2e-2, so the bound stays."""
    for kv in (None, "fp8"):
        graph, eager = graph_vs_eager(name, kv)
        _close(graph, eager, LOGIT_TOL, LOGIT_TOL, f"{name} kv={kv}: graph vs eager step logits")


@pytest.fixture
def caches(monkeypatch):
    """Every ``KVCache`` built while the test runs (``generate()`` makes one per call, directly or
    through its ``GraphDecoder``), in order."""
    from gke_ray_train_amd.models import generation as G
    made = []

    class Spy(G.KVCache):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(G, "KVCache", Spy)
    return made


def _one_fp8_cache(caches, n):
    """The single cache of the last ``generate()`` call: fp8 mode, codes and scales written for the
    first ``n`` slots of row 0 in every layer. Clears the list."""
    assert len(caches) == 1, len(caches)
    c = caches.pop()
    assert c.fp8 and c.k[0].dtype == torch.uint8 and c.k_scale[0].dtype == torch.float32
    for li in range(len(c.k)):
        assert bool(c.k_scale[li][0, :n].gt(0).all()) and bool(c.v_scale[li][0, :n].gt(0).all()), li
        assert bool(c.k[li][0, :n].ne(0).any(-1).all())


@pytest.mark.parametrize("name", MODELS)
def test_generate_builds_an_fp8_cache_in_every_mode(name, caches):
    """``generate(kv_cache_dtype="fp8")`` observed at the cache it builds, for every decode path:
    graph + device loop, graph + host loop, eager, sampled, padded batch, prompt lookup on each of
    the three loops. The greedy graph run's tokens are those of a hand-driven fp8 ``GraphDecoder``
    (the same kernels), so the cache is also the one that is decoded from."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    ids = _ids(m, 2, 12, 5)
    new = 10
    kw = dict(max_new_tokens=new, kv_cache_dtype="fp8")
    dev = m.generate(ids, use_graph=True, device_loop=True, **kw)
    _one_fp8_cache(caches, 12 + new - 1)
    host = m.generate(ids, use_graph=True, device_loop=False, **kw)
    _one_fp8_cache(caches, 12 + new - 1)
    assert dev.shape == (2, 22) and torch.equal(dev, host)
    dec = G.GraphDecoder(m, 2, 12 + new, kv_cache_dtype="fp8")
    caches.pop()
    lg, toks = dec.prefill(ids), []
    for t in range(new):
        toks.append(lg.argmax(-1))
        if t + 1 < new:
            lg = dec.step(toks[-1])
    assert torch.equal(host[:, 12:], torch.stack(toks, 1))
    eager = m.generate(ids, use_graph=False, **kw)
    _one_fp8_cache(caches, 12 + new - 1)
    assert eager.shape == (2, 22) and torch.equal(eager[:, :12], ids)
    samp = m.generate(ids, do_sample=True, top_k=20, seed=3, **kw)
    _one_fp8_cache(caches, 12 + new - 1)
    assert samp.shape == (2, 22)
    mask = torch.ones_like(ids)
    mask[1, :5] = 0
    for graph in (True, False):
        out = m.generate(ids, attention_mask=mask, use_graph=graph, **kw)
        _one_fp8_cache(caches, 12 + new - 1)
        assert out.shape == (2, 22)
    for graph, loop in ((True, True), (True, False), (False, None)):
        out = m.generate(ids[:1], use_graph=graph, device_loop=loop, prompt_lookup_num_tokens=2, **kw)
        _one_fp8_cache(caches, 12 + new - 1)
        assert out.shape == (1, 22)
    m.generate(ids, max_new_tokens=new)       # the default still builds the bf16 cache
    assert len(caches) == 1 and not caches[0].fp8 and caches[0].k[0].dtype == torch.bfloat16


@pytest.mark.parametrize("name", MODELS)
def test_left_padded_batch_matches_each_row_alone(name):
    """Lengths (9, 4), left-padded: each row's step logits against that row run alone at the same
    row count (its prompt repeated), teacher-forced with the alone run's tokens."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    steps, L = 6, 24
    prompts = [_ids(m, 1, 9, 11)[0], _ids(m, 1, 4, 12)[0]]
    ref = []
    for b, p in enumerate(prompts):
        dec = G.GraphDecoder(m, 2, L, kv_cache_dtype="fp8")
        out = [dec.prefill(p[None].repeat(2, 1)).clone()]
        for _ in range(steps):
            out.append(dec.step(out[-1].argmax(-1)).clone())
        ref.append(torch.stack(out)[:, b])
    ref = torch.stack(ref, 1)                                   # [steps + 1, 2, V]
    toks = ref.argmax(-1)
    ids = _ids(m, 2, 9, 13)
    mask = torch.ones_like(ids)
    ids[0], ids[1, 5:], mask[1, :5] = prompts[0], prompts[1], 0
    dec = G.GraphDecoder(m, 2, L, kv_cache_dtype="fp8")
    got = [dec.prefill(ids, mask).clone()]
    for t in range(steps):
        got.append(dec.step(toks[t]).clone())
    _close(torch.stack(got), ref, LOGIT_TOL, LOGIT_TOL, f"{name}: fp8 padded batch vs each row alone")


@pytest.mark.parametrize("name", MODELS)
def test_prompt_lookup_with_forced_acceptance(name):
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    ids = _ids(m, 1, 16, 7)
    new = 13
    plain = m.generate(ids, max_new_tokens=new, use_graph=True, kv_cache_dtype="fp8")
    G.last_spec_stats.update(n_replays=0, n_emitted=0)
    spec = m.generate(ids, max_new_tokens=new, use_graph=True, kv_cache_dtype="fp8", prompt_lookup_num_tokens=3,
                      _spec_plan=plain[0, 16:].clone(), sync_every=1)
    print(f"{name}: {G.last_spec_stats}")
    assert torch.equal(spec, plain), (spec[0, 16:].tolist(), plain[0, 16:].tolist())
    assert G.last_spec_stats["n_emitted"] == new and G.last_spec_stats["n_replays"] < new - 1


def test_generate_from_an_nf4_base():
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    m = build_llama("llama-tiny-gqa", device=DEV, dtype=torch.bfloat16, seed=0, intermediate_size=1536)
    quantize_model_(m, BitsAndBytesConfig())
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16)).eval()
    ids = torch.randint(0, 512, (2, 40), device=DEV, generator=_gen(7))
    out = pm.generate(ids, max_new_tokens=8, use_graph=True, kv_cache_dtype="fp8")
    assert out.shape == (2, 48) and torch.equal(out[:, :40], ids)
    dec = G.GraphDecoder(pm.base_model, 2, 64, kv_cache_dtype="fp8")
    lg = dec.prefill(ids)
    for _ in range(8):
        lg = dec.step(lg.argmax(-1))
    assert torch.isfinite(lg).all()


@pytest.mark.parametrize("name", MODELS)
def test_chunked_prefill_takes_the_dequantising_path(name):
    """A chunk of more than 4 tokens on a non-empty fp8 cache: append, dequantise rows [0, n), flash
    kernel. The same 8 tokens fed as two chunks of 4 go through the fp8 decode kernel over the same
    kind of cache: two decode paths, compared at the 2e-2 bound between decode paths."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    ids = _ids(m, 1, 20, 9)
    outs = []
    for chunks in ((8,), (4, 4)):
        c = G.KVCache(m.config, 1, 32, DEV, "fp8")
        G.forward_cached(m, ids[:, :12], c)
        at = 12
        for n in chunks:
            lg = G.forward_cached(m, ids[:, at:at + n], c)
            at += n
        assert c.len == 20
        outs.append(lg)
    _close(outs[0], outs[1], LOGIT_TOL, LOGIT_TOL, f"{name}: chunked prefill, dequantising path vs decode kernel")


def _child():
    from gke_ray_train_amd.models import generation as G
    from gke_ray_train_amd.ops import fused
    assert not fused._DECODE_KERNEL
    m = _model("llama-tiny-d64")
    ids = _ids(m, 1, 8, 0)
    for call in (lambda: m.generate(ids, max_new_tokens=2, kv_cache_dtype="fp8"),
                 lambda: m.generate(ids, max_new_tokens=2, kv_cache_dtype="fp8", use_graph=False),
                 lambda: G.GraphDecoder(m, 1, 16, kv_cache_dtype="fp8")):
        try:
            call()
        except ValueError as e:
            assert "GRT_DECODE_ATTN" in str(e) and "fp8" in str(e), e
        else:
            raise AssertionError("fp8 cache with GRT_DECODE_ATTN=0 did not raise")
    assert m.generate(ids, max_new_tokens=2).shape == (1, 10)   # the bf16 cache still decodes
    print("child ok")


def test_decode_attn_switch_off_with_fp8_raises_in_child():
    env = dict(os.environ, GRT_DECODE_ATTN="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, f"child exited with {r.returncode}:\n{r.stdout}"


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
