"""fp8 KV cache on the CPU: the format's host definition (``ops/_ref.py::kv_fp8_*``) against torch's
own e4m3fn cast, its elementwise error bound, and the cache wired through ``forward_cached`` /
``generate`` on the tiny fp32 Llama of test_generation_cpu.py (the ``_ref`` path of the feature).

The bound of the format, per element: |dequant - x| <= max(|x| 2^-4, scale 2^-10), half an ulp of 3
mantissa bits or half the subnormal step 2^-9 (in units of the vector's scale)."""
import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models import generation as G
from gke_ray_train_amd.ops import _ref

CPU = torch.device("cpu")


def fp8_bound(x, scale):
    return torch.maximum(x.float().abs() * 2.0 ** -4, scale.unsqueeze(-1) * 2.0 ** -10)


def tie_vectors(D=64):
    """bf16 vectors [n, D] that each contain 448 (so their scale is exactly 1) and between them hold
    every finite code's value, every midpoint between neighbouring codes (exact in bf16: one more
    mantissa bit than e4m3) and each midpoint +- one bf16 ulp, in both signs."""
    tab = _ref.kv_fp8_table()
    pos = tab[:127]                                  # 0 ... 448, ascending
    mid = (pos[:-1] + pos[1:]) / 2
    assert torch.equal(mid.bfloat16().float(), mid)
    mb = mid.bfloat16()
    up = (mb.view(torch.int16) + 1).view(torch.bfloat16)
    dn = (mb.view(torch.int16) - 1).view(torch.bfloat16)
    vals = torch.cat([pos.bfloat16(), mb, up, dn])
    vals = torch.cat([vals, -vals])
    per = D - 1
    pad = (-len(vals)) % per
    vals = torch.cat([vals, vals.new_zeros(pad)]).view(-1, per)
    return torch.cat([torch.full((vals.shape[0], 1), 448.0, dtype=torch.bfloat16), vals], 1)


def test_quantizer_matches_torch_e4m3fn_cast_on_codes_ties_and_neighbours():
    x = tie_vectors()
    codes, scale = _ref.kv_fp8_quantize(x)
    assert torch.equal(scale, torch.ones_like(scale))
    want = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want)
    assert not ((codes & 0x7F) == 0x7F).any()                          # no NaN code
    assert set(codes.flatten().tolist()) >= set(range(127)) | set(range(128, 255))  # all 254 finite codes
    # the midpoints tie to the even code
    tab = _ref.kv_fp8_table()
    mid = (tab[:126] + tab[1:127]) / 2
    mc, _ = _ref.kv_fp8_quantize(torch.cat([torch.tensor([448.0]), mid]).bfloat16())
    assert (mc[1:] % 2 == 0).all()
    assert torch.equal(_ref.kv_fp8_dequantize(codes, scale), tab[codes.long()])


def test_zero_vector_gives_code_zero_and_scale_one():
    codes, scale = _ref.kv_fp8_quantize(torch.zeros(3, 64, dtype=torch.bfloat16))
    assert torch.equal(codes, torch.zeros(3, 64, dtype=torch.uint8))
    assert torch.equal(scale, torch.ones(3))


def test_table_is_the_e4m3fn_code_table():
    tab = _ref.kv_fp8_table()
    assert tab.shape == (256,) and tab[126] == 448.0 and tab[1] == 2.0 ** -9 and tab[8] == 2.0 ** -6
    assert torch.isnan(tab[127]) and torch.isnan(tab[255]) and torch.isfinite(tab[:127]).all()
    assert torch.equal(tab[128:255], -tab[:127])


@pytest.mark.parametrize("D", [64, 128])
def test_elementwise_bound_on_randn(D):
    x = torch.randn(4096, D, generator=torch.Generator().manual_seed(D)).bfloat16()
    codes, scale = _ref.kv_fp8_quantize(x)
    assert not ((codes & 0x7F) == 0x7F).any()
    assert ((codes & 0x7F) == 126).any(-1).all()       # every vector's largest element is code 126
    assert torch.equal(scale, x.float().abs().amax(-1) / 448)
    err = (_ref.kv_fp8_dequantize(codes, scale) - x.float()).abs()
    assert (err <= fp8_bound(x, scale)).all()


def _tiny(seed=0):
    return build_llama("llama-tiny-gqa", device="cpu", dtype=torch.float32, seed=seed).eval()


def _prefill_pair(m, ids, mask=None, max_len=16):
    B = ids.shape[0]
    plain = G.KVCache(m.config, B, max_len, CPU, torch.float32)
    fp8 = G.KVCache(m.config, B, max_len, CPU, "fp8")
    with torch.no_grad():
        lp = G.forward_cached(m, ids, plain, mask)
        lf = G.forward_cached(m, ids, fp8, mask)
    return plain, fp8, lp, lf


def _check_rows(plain, fp8, lens):
    for li in range(len(plain.k)):
        for codes, scale, ref in ((fp8.k[li], fp8.k_scale[li], plain.k[li]), (fp8.v[li], fp8.v_scale[li], plain.v[li])):
            assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
            for b, n in enumerate(lens):
                deq = _ref.kv_fp8_dequantize(codes[b, :n], scale[b, :n])
                assert ((deq - ref[b, :n]).abs() <= fp8_bound(ref[b, :n], scale[b, :n])).all(), (li, b)


def test_prefill_logits_equal_plain_cache_and_rows_within_bound():
    m = _tiny()
    ids = torch.randint(0, m.config.vocab_size, (2, 7), generator=torch.Generator().manual_seed(0))
    plain, fp8, lp, lf = _prefill_pair(m, ids)
    assert fp8.fp8 and not plain.fp8 and fp8.len == plain.len == 7
    assert torch.equal(lp, lf)
    _check_rows(plain, fp8, [7, 7])


@pytest.mark.parametrize("side", ["left", "right"])
def test_padded_prefill_logits_equal_and_own_slots_within_bound(side):
    m = _tiny()
    ids = torch.randint(0, m.config.vocab_size, (2, 5), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(2, 5, dtype=torch.long)
    if side == "left":
        mask[1, :3] = 0
    else:
        mask[1, 2:] = 0
    plain, fp8, lp, lf = _prefill_pair(m, ids, mask)
    assert torch.equal(lp, lf)
    assert fp8.lens.tolist() == [5, 2]
    _check_rows(plain, fp8, [5, 2])


def _step_diff(seed):
    m = _tiny(seed)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, m.config.vocab_size, (2, 7), generator=g)
    nxt = torch.randint(0, m.config.vocab_size, (2, 1), generator=g)
    plain, fp8, _, _ = _prefill_pair(m, ids)
    with torch.no_grad():
        sp = G.forward_cached(m, nxt, plain)
        sf = G.forward_cached(m, nxt, fp8)
    return (sp - sf).abs().max().item(), sp.abs().max().item()


STEP_BOUND = 2 * 0.03754


def test_decode_step_uses_the_quantised_cache_and_stays_close():
    """One decode step after the prefill: the logits differ from the plain cache's (the quantised
    rows are what is read) and stay within twice the worst difference measured over three seeds.
    Measured on the CPU (max |logit difference|, with max |logit| beside it): seed 0 0.03329 (1.49),
    seed 1 0.03754 (1.37), seed 2 0.03159 (1.38). Code flips are discrete and seed-dependent, hence
    the factor 2: the bound is 0.07508."""
    for seed in (0, 1, 2):
        d, top = _step_diff(seed)
        print(f"seed {seed}: max |logit diff| {d:.4g}, max |logit| {top:.4g}")
        assert 0.0 < d <= STEP_BOUND


@pytest.fixture
def caches(monkeypatch):
    """Every ``KVCache`` that ``generate()`` builds, in order."""
    made = []

    class Spy(G.KVCache):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(G, "KVCache", Spy)
    return made


def _manual_greedy(m, ids, new, dtype):
    """Greedy tokens from a hand-written ``forward_cached`` loop over a cache of ``dtype``, and the
    logits each was picked from."""
    cache = G.KVCache(m.config, ids.shape[0], ids.shape[1] + new, CPU, dtype)
    toks, logits = [], []
    with torch.no_grad():
        lg = G.forward_cached(m, ids, cache)
        for t in range(new):
            logits.append(lg)
            toks.append(lg.argmax(-1))
            if t + 1 < new:
                lg = G.forward_cached(m, toks[-1][:, None], cache)
    return torch.stack(toks, 1), torch.stack(logits, 1)


def test_generate_fp8_builds_an_fp8_cache_and_decodes_from_it(caches):
    """``generate(kv_cache_dtype="fp8")`` is observed at the cache: the one it builds is in fp8 mode
    and holds codes, and its tokens are those of a manual loop over ``KVCache(..., "fp8")``, whose
    step logits are not the plain cache's."""
    m = _tiny()
    ids = torch.tensor([[3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4]])
    a = G.generate(m, ids, max_new_tokens=8, kv_cache_dtype="fp8")
    assert a.shape == (1, 19) and torch.equal(a[:, :11], ids)
    assert len(caches) == 1 and caches[0].fp8 and caches[0].k[0].dtype == torch.uint8
    assert caches[0].len == 18 and bool(caches[0].k_scale[0][0, :18].ne(0).all())
    toks, lf = _manual_greedy(m, ids, 8, "fp8")
    assert torch.equal(a[:, 11:], toks)
    _, lp = _manual_greedy(m, ids, 8, torch.float32)
    assert torch.equal(lf[:, 0], lp[:, 0]) and not torch.equal(lf[:, 1], lp[:, 1])
    del caches[:]
    for kw in (dict(kv_cache_dtype="fp8_e4m3"), dict(kv_cache_dtype="fp8", prompt_lookup_num_tokens=2)):
        b = G.generate(m, ids, max_new_tokens=8, **kw)
        assert torch.equal(a, b), kw
    assert G.last_spec_stats["n_emitted"] == 8
    assert len(caches) == 2 and all(c.fp8 for c in caches)
    del caches[:]
    d = G.generate(m, ids, max_new_tokens=8, kv_cache_dtype="auto")
    assert torch.equal(d, G.generate(m, ids, max_new_tokens=8))
    assert len(caches) == 2 and not any(c.fp8 for c in caches) and caches[0].k[0].dtype == torch.float32


def test_generate_refuses_an_unknown_kv_cache_dtype():
    m = _tiny()
    ids = torch.tensor([[3, 4, 5]])
    with pytest.raises(ValueError, match="kv_cache_dtype.*fp8"):
        G.generate(m, ids, max_new_tokens=2, kv_cache_dtype="int3")


def test_nbytes_ratio():
    cfg = _tiny().config
    D = cfg.head_dim
    bf = G.KVCache(cfg, 2, 24, CPU, torch.bfloat16)
    f8 = G.KVCache(cfg, 2, 24, CPU, "fp8")
    assert bf.nbytes() == cfg.num_hidden_layers * 2 * 2 * 24 * cfg.num_key_value_heads * D * 2
    assert f8.nbytes() * 2 * D == bf.nbytes() * (D + 4)
    assert f8.k_scale[0].shape == (2, 24, cfg.num_key_value_heads) and f8.k[0].shape == (2, 24, cfg.num_key_value_heads, D)
