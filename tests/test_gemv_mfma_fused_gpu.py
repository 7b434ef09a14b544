"""The MFMA skinny GEMM with the decode step's prologues / epilogues (gemv_mfma_fused.hip, binding
``gemv_mfma_fused``) and the norm-fused decode step at 3+ rows. References are float64 math rounded
where the kernel rounds; the comparison and its bounds are ``test_kernels_gpu.py``'s for ``gemv_fused``
(2e-2 against fp32 math, 1e-2 for the RoPE epilogue), the logit bound ``test_decode_d64_gpu.py``'s.
``g`` with ``res`` is refused as in ``gemv_fused`` (a kernel that reads an accumulator set cannot zero
it for the next producer), so norm-on-load into the residual epilogue is tested as a chained pair."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kernels_gpu as base  # noqa: E402  (_C, _close)

pytestmark = pytest.mark.gpu
DEV, EPS, LOGIT_TOL, BF = "cuda", 1e-5, 2e-2, torch.bfloat16
MS = [3, 5, 16]  # unused A rows; a row in the second accumulator group; a full tile
NK = [(40, 256), (40, 768), (16392, 256)]  # column tail; uneven K split; 4 waves (N > 16384)


def _ref(x, w, nw=None, swiglu=False):
    """bf16(A W^T) in float64, A = x, bf16(rms_norm(x) nw) or bf16(silu(gate) up); and the
    accumulator pair whose set 1 holds 2^20 sum(x^2) per row, spread over the 64 slots."""
    a, K = x.double(), w.shape[1]
    acc = torch.zeros(2, x.shape[0], 64, dtype=torch.int64, device=DEV)
    tot = torch.round(a.pow(2).sum(-1) * 2 ** 20).long()
    acc[1] = (tot // 64)[:, None]
    acc[1, :, 7] += tot % 64
    if nw is not None:
        a = (a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + EPS) * nw.double()).to(BF).double()
    if swiglu:
        a = (torch.nn.functional.silu(a[:, :K]) * a[:, K:]).to(BF).double()
    return (a @ w.double().t()).to(BF), acc


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("case", ["normx", "res", "swi_res", "res_then_normx"])
def test_projection(M, N, K, case):
    C, swi = base._C(), case == "swi_res"
    if case == "res_then_normx":  # the producer's N is the consumer's K: the next multiple of 256
        N = -(-N // 256) * 256
    g = torch.Generator(device=DEV).manual_seed(M * N + K)
    x = torch.randn(M, (2 if swi else 1) * K, device=DEV, dtype=BF, generator=g)
    w = torch.randn(N, K, device=DEV, dtype=BF, generator=g) * 0.02
    res = torch.randn(M, N, device=DEV, dtype=BF, generator=g)
    if case == "normx":
        nw = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF)
        y, acc = _ref(x, w, nw)
        return base._close(C.gemv_mfma_fused(x, w, acc, 1, g=nw, eps=EPS), y, 2e-2, 2e-2, case)
    ref = (_ref(x, w, swiglu=swi)[0].double() + res.double()).to(BF)
    runs = []
    for slot in (0, 1, 0):
        acc = torch.full((2, M, 64), 12345, dtype=torch.int64, device=DEV)
        acc[slot] = 0
        h = C.gemv_mfma_fused(x, w, acc, slot, swiglu=swi, res=res)
        base._close(h, ref, 2e-2, 2e-2, case)
        assert int(acc[1 - slot].abs().sum()) == 0
        # Per workgroup (16 columns) and row: the h^2 are exact in fp32 (8-bit significands), their sum is
        # a 4-level tree of fp32 adds (relative error <= 4 * 2^-24), the scaling by 2^20 is exact, llrintf is
        # off by <= 1/2 unit (one allowed): |slots - 2^20 sum(h^2)| <= ceil(N / 16) + 2^-22 exact, h as written
        exact = h.double().pow(2).sum(-1) * 2 ** 20
        assert ((acc[slot].sum(-1).double() - exact).abs() <= (N + 15) // 16 + exact * 2.0 ** -22).all()
        runs.append((h, acc[slot].clone()))
    assert all(torch.equal(h, runs[0][0]) and torch.equal(s, runs[0][1]) for h, s in runs[1:])
    if case == "res_then_normx":  # the consumer reads what the producer left (set 0)
        w2 = torch.randn(40, N, device=DEV, dtype=BF, generator=g) * 0.02
        nw = (1 + 0.1 * torch.randn(N, device=DEV, generator=g)).to(BF)
        base._close(C.gemv_mfma_fused(h, w2, acc, 0, g=nw, eps=EPS), _ref(h, w2, nw)[0], 2e-2, 2e-2, case)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("hd,normx", [(64, True), (64, False), (128, True), (128, False)])
def test_rope_epilogue(M, K, hd, normx):
    """q, k rotated, k / v in cache slot pos[m] of row m, nothing else written (positions -1, >= L: nothing)."""
    C, L, hq, hkv, half = base._C(), 24, 4, 2, hd // 2
    g = torch.Generator(device=DEV).manual_seed(M * K + hd + normx)
    h = torch.randn(M, K, device=DEV, dtype=BF, generator=g)
    w = torch.randn((hq + 2 * hkv) * hd, K, device=DEV, dtype=BF, generator=g) * 0.02
    nw = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF)
    ang = torch.arange(2 * L, device=DEV, dtype=torch.float32)[:, None] * torch.rand(half, device=DEV, generator=g)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    pos = ((torch.arange(M, device=DEV) * 5 + 2) % L).int()  # distinct per row
    pos[1], pos[2] = -1, L + 3
    kc0 = torch.randn(M, L, hkv, hd, device=DEV, dtype=BF, generator=g)
    vc0 = torch.randn(M, L, hkv, hd, device=DEV, dtype=BF, generator=g)
    kc, vc = kc0.clone(), vc0.clone()
    qkv, acc = _ref(h, w, nw if normx else None)
    q = C.gemv_mfma_fused(h, w, acc, 1, cos=cos, sin=sin, pos=pos, kc=kc, vc=vc, hq=hq, hkv=hkv,
                          **(dict(g=nw, eps=EPS) if normx else {}))
    qkv = qkv.float().view(M, hq + 2 * hkv, hd)
    ok, p = (pos >= 0) & (pos < L), pos.clamp(0, L - 1).long()
    cs, sn = cos[p][:, None], sin[p][:, None]  # [M, 1, half] fp32
    rot = torch.cat([qkv[..., :half] * cs - qkv[..., half:] * sn, qkv[..., half:] * cs + qkv[..., :half] * sn], -1)
    rows = torch.arange(M, device=DEV)[ok]
    kr, vr, kept = kc0.clone(), vc0.clone(), torch.ones(M, L, dtype=torch.bool, device=DEV)
    kr[rows, p[ok]], vr[rows, p[ok]], kept[rows, p[ok]] = rot[ok, hq:hq + hkv].to(BF), qkv[ok, hq + hkv:].to(BF), False
    base._close(q[ok], rot[ok, :hq], 1e-2, 1e-2, "q")
    base._close(kc, kr, 1e-2, 1e-2, "k cache")
    base._close(vc, vr, 2e-2, 2e-2, "v cache")
    assert torch.equal(kc[kept], kc0[kept]) and torch.equal(vc[kept], vc0[kept])
    assert (kc[~kept] != kc0[~kept]).float().mean() > 0.9 and (vc[~kept] != vc0[~kept]).float().mean() > 0.9


def test_refusals():
    C = base._C()
    acc = torch.zeros(2, 17, 64, dtype=torch.int64, device=DEV)
    for M, K in ((2, 256), (17, 256), (3, 264)):  # 264: a multiple of 8, so the K % 256 rule refuses it
        with pytest.raises(RuntimeError, match="3..16 rows, K % 256"):
            C.gemv_mfma_fused(torch.zeros(M, K, device=DEV, dtype=BF), torch.zeros(32, K, device=DEV, dtype=BF), acc, 0,
                              g=torch.ones(K, device=DEV, dtype=BF))
    x, w = torch.zeros(3, 256, device=DEV, dtype=BF), torch.zeros(384, 256, device=DEV, dtype=BF)
    res, cos = torch.zeros(3, 384, device=DEV, dtype=BF), torch.ones(4, 32, device=DEV)
    kc = torch.zeros(3, 4, 2, 64, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="RoPE epilogue is for the qkv"):
        C.gemv_mfma_fused(x, w, acc, 0, res=res, cos=cos, sin=cos.clone(), kc=kc, vc=kc.clone(), hq=2, hkv=2,
                          pos=torch.zeros(3, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="g .normalise the input. or res"):
        C.gemv_mfma_fused(x, w, acc, 0, g=torch.ones(256, device=DEV, dtype=BF), res=res)


# (config, intermediate size % 256 == 0, seed of model and prompts): of seeds 0-79 the one with the most
# decisive eager steps (top-1 / top-2 margin over twice the tolerance) at B = 3 and 8 together (d64: 31
# of 48 at B = 8, 15 of 18 at B = 3, either cache; gqa: 32 of 48, 13 of 18). lens: a left-padded batch.
D64, GQA = ("llama-tiny-d64", 768, 16), ("llama-tiny-gqa", 1536, 54)


@pytest.mark.parametrize("model,B,kv,lens", [(D64, 3, None, None), (D64, 8, None, None), (GQA, 3, None, None),
                                             (GQA, 8, None, None), (D64, 3, "fp8", None), (GQA, 3, None, [5, 12, 9])])
def test_decode_step(monkeypatch, model, B, kv, lens):
    """With the row limit raised (2: the step measured slower than the generic one) the captured step is
    the norm-fused one; teacher-forced logits == eager ``forward_cached``, or == every row decoded alone."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    monkeypatch.setattr(G, "GEMV_MFMA_FUSED_MAX_ROWS", 16)
    (name, inter, seed), steps, S, L = model, 6, 12, 32
    m = build_llama(name, device=DEV, dtype=BF, seed=seed, intermediate_size=inter).eval()
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids, mask = torch.randint(0, m.config.vocab_size, (8, S), device=DEV, generator=g)[:B], None
    if lens is None:
        cache = G.KVCache(m.config, B, L, DEV, "fp8" if kv else BF)
        ref = [G.forward_cached(m, ids, cache)]
        for _ in range(steps):
            ref.append(G.forward_cached(m, ref[-1].argmax(-1)[:, None], cache))
        ref = torch.stack(ref)
    else:
        mask, rows = torch.zeros_like(ids), []
        for b, n in enumerate(lens):
            mask[b, S - n:] = 1
            one = G.GraphDecoder(m, 1, L)
            rows.append([one.prefill(ids[b:b + 1, S - n:]).clone()])
            for _ in range(steps):
                rows[-1].append(one.step(rows[-1][-1].argmax(-1)).clone())
        ref = torch.stack([torch.cat(r) for r in rows], 1)  # [steps + 1, B, V]
    dec = G.GraphDecoder(m, B, L, kv_cache_dtype=kv)
    assert dec.norm_ws is not None
    lg = torch.stack([dec.prefill(ids, mask).clone()] + [dec.step(ref[t].argmax(-1)).clone() for t in range(steps)])
    top2 = ref[1:].topk(2, -1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2 * (LOGIT_TOL + LOGIT_TOL * top2[..., 0].abs())
    assert lens is not None or decisive.float().mean().item() >= 0.5, "pick a seed with decisive greedy steps"
    base._close(lg, ref, LOGIT_TOL, LOGIT_TOL, "graph decoder logits")
    assert torch.equal(lg[1:].argmax(-1)[decisive], ref[1:].argmax(-1)[decisive])
