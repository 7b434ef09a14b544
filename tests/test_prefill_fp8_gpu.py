"""Flash prefill over the fp8 KV cache (prefill_attention_fp8.hip, ``ops.prefill_attention_fp8``) against
float64 softmax attention over ``table[code] * scale``, and ``prefill_chunk_size`` of ``generate()`` on
the two tiny models of test_kv_fp8_gpu.py, whose comparison rule this file copies: ``_close`` with the
attention tolerance 1e-2 / 1e-2 (under 0.1 % of the elements past it, none past 10x), 2e-2 / 2e-2 for
logits between decode paths. The token rule: the S query tokens of a row are the last S of its n keys,
token t attends keys [0, n - (S - 1 - t))."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOGIT_TOL = 2e-2
MODELS = ["llama-tiny-gqa", "llama-tiny-d64"]   # head_dim 128 and 64
_cache = {}


def _close(a, b, atol, rtol, what=""):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.4g}, worst element at {worst:.3f}x its tolerance")
    assert not torch.isnan(a).any(), f"{what}: NaN in kernel output"
    assert (err > tol).float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"


def _case(D, G, S, n, B=2, hkv=2, L=None):
    """Host inputs of one case (seeded by its shape) and their float64 reference, computed once. The
    cache holds L > n slots. Per-token magnitudes: K 2^-2 .. 2^2 (16x), V 1e-4 .. 1 (four orders; the
    largest is the level of the randn inputs the 1e-2 / 1e-2 tolerance was set for), so a dropped or
    swapped scale is off by orders of magnitude."""
    from gke_ray_train_amd.ops import _ref
    key = (D, G, S, n, L)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * D + 100 * G + 7 * S + n)
        L = L or n + 9
        q = torch.randn(B, S, hkv * G, D, generator=g).bfloat16()
        kmag = 2.0 ** (torch.rand(B, L, hkv, 1, generator=g) * 4 - 2)
        vmag = 10.0 ** (torch.rand(B, L, hkv, 1, generator=g) * -4)
        (kc, ks), (vc, vs) = (_ref.kv_fp8_quantize((torch.randn(B, L, hkv, D, generator=g) * mag).bfloat16())
                              for mag in (kmag, vmag))
        tab = _ref.kv_fp8_table().double()
        kd, vd = ((tab[c[:, :n].long()] * s[:, :n].double().unsqueeze(-1)).repeat_interleave(G, 2)
                  for c, s in ((kc, ks), (vc, vs)))
        s = torch.einsum("bthd,bjhd->bhtj", q.double(), kd) * D ** -0.5
        hidden = torch.arange(n)[None, :] > torch.arange(S)[:, None] + (n - S)
        ref = torch.einsum("bhtj,bjhd->bthd", torch.softmax(s.masked_fill(hidden, float("-inf")), -1), vd)
        assert torch.isfinite(ref).all()
        _cache[key] = tuple(t.to(DEV) for t in (q, kc, ks, vc, vs, ref))
    return _cache[key]


def _run(q, kc, ks, vc, vs, n):
    from gke_ray_train_amd import ops
    return ops.prefill_attention_fp8(q, kc[:, :n], vc[:, :n], ks[:, :n], vs[:, :n])


# (5, 5): n == S, token 0 sees one key; (5, 70): past the decode kernel's T limit; (33, 64 / 65): second
# 32-row tile, key-tile edge; (129, ...): second workgroup at G = 1, the diagonal crosses key tiles
SHAPES = [(5, 5), (5, 70), (33, 64), (33, 65), (64, 200), (129, 129), (129, 300)]


@pytest.mark.parametrize("S,n", SHAPES)
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_matches_float64(D, G, S, n):
    q, kc, ks, vc, vs, ref = _case(D, G, S, n)
    o = _run(q, kc, ks, vc, vs, n)
    assert o.shape == q.shape and o.dtype == torch.bfloat16 and o.is_contiguous()
    _close(o, ref, 1e-2, 1e-2, f"fp8 prefill attention D={D} G={G} S={S} n={n}")


@pytest.mark.parametrize("D", [64, 128])
def test_slots_past_n_are_never_read(D):
    """n = 70 ends inside the second key tile: NaN codes and scales in every slot past n change no bit."""
    S, n = 37, 70
    q, kc, ks, vc, vs, ref = (t.clone() for t in _case(D, 4, S, n, L=160))
    outs = []
    for code, scale in ((0x7F, float("nan")), (0, 0.0)):
        for c, s in ((kc, ks), (vc, vs)):
            c[:, n:], s[:, n:] = code, scale
        outs.append(_run(q, kc, ks, vc, vs, n))
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])
    _close(outs[0], ref, 1e-2, 1e-2, f"poisoned cache D={D}")


@pytest.mark.parametrize("what", ["misaligned codes", "S > n", "G = 3", "fp32 q", "D = 96"])
def test_binding_refusals(what):
    from gke_ray_train_amd import ops
    B, S, n, hkv, D = 1, 6, 12, 2, 96 if what == "D = 96" else 64
    q = torch.zeros(B, S, 6 if what == "G = 3" else 4, D, device=DEV, dtype=torch.bfloat16)
    kc = torch.zeros(B, n, hkv, D + 4, device=DEV, dtype=torch.uint8)
    kc = kc[..., :D] if what == "misaligned codes" else kc[..., :D].contiguous()   # head stride D + 4
    sc = torch.ones(B, n, hkv, device=DEV)
    if what == "S > n":
        kc, sc = kc[:, :S - 1], sc[:, :S - 1]
    q = q.float() if what == "fp32 q" else q
    match = {"misaligned codes": "8-byte aligned", "S > n": "S = 6, n = 5", "G = 3": "GQA group.*3",
             "fp32 q": "torch.float32", "D = 96": "head_dim 96"}[what]
    with pytest.raises((RuntimeError, ValueError), match=match):
        ops.prefill_attention_fp8(q, kc, kc.clone() if what != "misaligned codes" else kc, sc, sc)


def _model(name):
    from gke_ray_train_amd.models import build_llama
    if name not in _cache:
        _cache[name] = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=0).eval()
    return _cache[name]


def _ids(m, B, S, seed):
    return torch.randint(0, m.config.vocab_size, (B, S), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("name", MODELS)
def test_forward_cached_chunk_matches_the_ref_path(name):
    """A 12-token prefill, then one 8-token chunk on the fp8 cache: the kernel path against the same
    calls on the CPU (``_ref`` quantiser, dequantised rows, math attention) with the same weights."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    cpu = build_llama(name, device="cpu", dtype=torch.bfloat16, seed=0).eval()
    cpu.load_state_dict(m.state_dict())
    ids = _ids(m, 2, 20, 21)
    out = []
    for model, dev, x in ((m, DEV, ids), (cpu, "cpu", ids.cpu())):
        c = G.KVCache(model.config, 2, 32, dev, "fp8")
        G.forward_cached(model, x[:, :12], c)
        out.append(G.forward_cached(model, x[:, 12:], c).to(DEV))
    _close(out[0], out[1], LOGIT_TOL, LOGIT_TOL, f"{name}: 8-token chunk on an fp8 cache, kernels vs _ref path")


@pytest.mark.parametrize("name", MODELS)
def test_generate_with_prefill_chunk_size(name):
    """Graph and eager ``generate`` with the prompt fed in chunks of 8 (20 tokens: 8, 8, 4). Their
    tokens agree up to the first near-tie: where they part, the two tokens' logits on the eager path
    lie within twice the 2e-2 bound between decode paths."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    ids = _ids(m, 2, 20, 22)
    kw = dict(prefill_chunk_size=8, kv_cache_dtype="fp8", max_new_tokens=4)
    a, b = m.generate(ids, **kw), m.generate(ids, use_graph=False, **kw)
    assert a.shape == b.shape == (2, 24) and torch.equal(a[:, :20], ids) and torch.equal(b[:, :20], ids)
    for r in range(2):
        diff = (a[r] != b[r]).nonzero()
        if len(diff):
            t = int(diff[0])
            c = G.KVCache(m.config, 1, 32, DEV, "fp8")
            lg = G._prefill(m, ids[r:r + 1], c, None, 8)[0]
            for tok in b[r, 20:t]:
                lg = G.forward_cached(m, tok.view(1, 1), c)[0]
            gap = (lg[a[r, t]] - lg[b[r, t]]).abs().item()
            print(f"{name} row {r}: paths part at token {t}, logit gap {gap:.4g}")
            assert gap <= 2 * LOGIT_TOL * (1 + lg.abs().max().item())
    mask = torch.ones_like(ids)
    mask[1, :3] = 0
    with pytest.raises(ValueError, match="prefill_chunk_size"):
        m.generate(ids, prefill_chunk_size=0, max_new_tokens=2)
    with pytest.raises(ValueError, match="one causal block"):
        m.generate(ids, prefill_chunk_size=8, attention_mask=mask, max_new_tokens=2)
