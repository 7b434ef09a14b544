"""``generate(..., attention_mask=...)`` on the GPU (bf16, head_dim 128 and 64): the public API drives
the decode kernels with unequal per-row positions and valid lengths (qkv GEMV RoPE epilogue /
``rope_append`` cache slots, split-K decode attention, the flash kernel's ``seqlens_k``, the device
sampler's per-row state) on every decode path.

The reference for row b of a padded batch is that row's unpadded prompt repeated B times, without a
mask, through the same kind of decoder: the same kernels at the same row count. Logits are compared
teacher-forced with the reference's greedy tokens at ``LOGIT_TOL`` (absolute plus relative), the
project's bound between decode paths (tests/test_decode_d64_gpu.py); end-to-end tokens are judged
against a no-cache forward with the rule of test_nf4_gemv_gpu.py::test_generate_from_nf4_base.
"""
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 12
ALL_LENS = [5, 12, 9]   # B = 2 takes the first two
STEPS = 6
LOGIT_TOL = 2e-2
# Seed of model and prompts, chosen from the reference runs alone (unpadded prompts, no mask): a
# random-init model's logits are nearly flat, and of seeds 0-79 these have the most steps whose
# reference top-1 / top-2 margin exceeds twice the tolerance, in every kind of decoder below
# (gqa: 10 of 12 at B = 2 and 13 of 18 at B = 3; d64: 12 of 12 and 16 of 18)
SEEDS = {"llama-tiny-gqa": 30, "llama-tiny-d64": 61}
MODELS = list(SEEDS)
KINDS = ["graph", "eager", "flash"]
_cache = {}


def _model(name, seed=None):
    from gke_ray_train_amd.models import build_llama
    seed = SEEDS[name] if seed is None else seed
    if (name, seed) not in _cache:
        _cache[name, seed] = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=seed).eval()
    return _cache[name, seed]


def _prompts(m, seed, lens=ALL_LENS):
    """The prompts and random valid ids for the pad columns (the same for every B)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    V = m.config.vocab_size
    prompts = [torch.randint(0, V, (n,), device=DEV, generator=g) for n in lens]
    fill = torch.randint(0, V, (len(lens), max(lens)), device=DEV, generator=g)
    return prompts, fill


def _left(prompts, fill):
    B, n = len(prompts), fill.shape[1]
    ids = fill[:B].clone()
    mask = torch.zeros_like(ids)
    for b, p in enumerate(prompts):
        ids[b, n - len(p):] = p
        mask[b, n - len(p):] = 1
    return ids, mask


def _close(a, b, atol, rtol, what=""):
    """The comparison of test_decode_d64_gpu.py: under 0.1 % of the elements past atol + rtol |ref|,
    and none past 10x that. Prints the worst error over its bound."""
    a, b = a.float(), b.float()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.4g}, worst element at {worst:.3f}x its tolerance")
    assert not torch.isnan(a).any(), f"{what}: NaN"
    assert (err > tol).float().mean().item() < 1e-3, f"{what}: max err {err.max().item():.4g} (mean {err.mean().item():.3g})"
    assert worst <= 10.0, f"{what}: an element is {worst:.1f}x its tolerance (max err {err.max().item():.4g})"


def _run(kind, m, ids, mask, toks, steps=STEPS, L=S + STEPS + 2):
    """Prefill + ``steps`` one-token steps of one kind of decoder with a cache of ``L`` slots;
    ``toks`` [steps, B] teacher-forces (None: the run's own greedy tokens). Returns the logits
    [steps + 1, B, V]."""
    from gke_ray_train_amd.models import generation as G
    from gke_ray_train_amd.ops import fused
    B = ids.shape[0]
    was = fused._DECODE_KERNEL
    fused._DECODE_KERNEL = kind != "flash"   # GRT_DECODE_ATTN=0: the flash forward kernel with seqlens_k
    try:
        if kind == "eager":
            cache = G.KVCache(m.config, B, L, DEV, torch.bfloat16)
            first = G.forward_cached(m, ids, cache, attention_mask=mask)

            def step(t):
                return G.forward_cached(m, t[:, None], cache)
        else:
            dec = G.GraphDecoder(m, B, L)
            first = dec.prefill(ids, mask)
            step = dec.step
        out = [first.clone()]
        for t in range(steps):
            out.append(step(out[-1].argmax(-1) if toks is None else toks[t]).clone())
    finally:
        fused._DECODE_KERNEL = was
    return torch.stack(out)


def _reference(kind, m, prompts, **kw):
    """Row b alone: its unpadded prompt repeated B times, no mask, greedy. Returns the logits
    [STEPS + 1, B, V] (row b of run b) and the greedy tokens [STEPS + 1, B]."""
    B = len(prompts)
    rows = [_run(kind, m, p[None].repeat(B, 1), None, None, **kw)[:, b] for b, p in enumerate(prompts)]
    ref = torch.stack(rows, 1)
    return ref, ref.argmax(-1)


def _decisive(ref):
    top2 = ref[1:].topk(2, -1).values      # the one-token steps
    margin = top2[..., 0] - top2[..., 1]
    return margin > 2 * (LOGIT_TOL + LOGIT_TOL * top2[..., 0].abs()), margin


def _check_ragged_logits(kind, name, B, seed=None, lens=ALL_LENS, **kw):
    seed = SEEDS[name] if seed is None else seed
    m = _model(name, seed)
    prompts, fill = _prompts(m, seed, lens)
    prompts = prompts[:B]
    ref, toks = _reference(kind, m, prompts, **kw)
    decisive, margin = _decisive(ref)
    print(f"decisive steps: {int(decisive.sum())} of {decisive.numel()}, margins {margin.flatten().tolist()}")
    assert decisive.float().mean().item() >= 0.5, "pick a seed with decisive greedy steps"
    ids, mask = _left(prompts, fill)
    got = _run(kind, m, ids, mask, toks, **kw)
    _close(got, ref, LOGIT_TOL, LOGIT_TOL, f"{name} B={B} {kind}: padded batch vs each row alone")
    assert torch.equal(got[1:].argmax(-1)[decisive], ref[1:].argmax(-1)[decisive])


# ------------------------------------------------------------------ 1. graph decoder
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_graph_decoder_ragged_logits(name, B):
    """B = 2 is the norm-fused step (RoPE epilogue of the qkv GEMV), B = 3 the unfused one
    (``rope_append``); both end in split-K decode attention with per-row valid lengths."""
    from gke_ray_train_amd.models import generation as G
    dec = G.GraphDecoder(_model(name), B, 16)
    assert (dec.norm_ws is not None) == (B == 2)
    _check_ragged_logits("graph", name, B)


# Prompts of 40 and 300 tokens: the cache is longer than the 256 keys up to which decode attention
# is one launch, so the step takes the split + combine kernels, and the short row leaves most of
# its splits empty. The reference runs use a cache of the same length (the same split of the keys).
LONG_LENS = [40, 300]
# chosen as SEEDS, of seeds 0-59 for these prompts (gqa: 12 of 12 decisive steps; d64: 11 of 12)
LONG_SEEDS = {"llama-tiny-gqa": 41, "llama-tiny-d64": 59}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_ragged_logits_past_the_one_launch_attention_length(name, kind):
    _check_ragged_logits(kind, name, 2, seed=LONG_SEEDS[name], lens=LONG_LENS, L=max(LONG_LENS) + STEPS + 2)


# ------------------------------------------------------------------ 2. eager, GRT_DECODE_ATTN=0
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("kind", ["eager", "flash"])
@pytest.mark.parametrize("name", MODELS)
def test_other_paths_ragged_logits(name, kind, B):
    _check_ragged_logits(kind, name, B)


def test_flash_kind_takes_the_flash_kernel(monkeypatch):
    """``_run("flash", ...)`` is the GRT_DECODE_ATTN=0 path: no decode-attention launch."""
    from gke_ray_train_amd import _native
    calls = {}
    C = _native.kernels()

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(C, name)
            if not callable(fn) or name.isupper():
                return fn

            def call(*a, **k):
                calls[name] = calls.get(name, 0) + 1
                return fn(*a, **k)
            return call

    monkeypatch.setattr(_native, "kernels", lambda: Proxy())
    m = _model("llama-tiny-d64")
    prompts, fill = _prompts(m, 1)
    ids, mask = _left(prompts[:2], fill)
    _run("flash", m, ids, mask, None, steps=2)
    assert calls.get("attn_fwd", 0) > 0 and "attn_decode_d64" not in calls and "attn_decode" not in calls, calls
    calls.clear()
    _run("graph", m, ids, mask, None, steps=2)
    assert calls.get("attn_decode_d64", 0) > 0, calls


# ------------------------------------------------------------------ 3. generate() end to end
def _judge(m, prompts, gen):
    """Each generated token of each row against a no-cache forward over that row's unpadded
    prefix: the chosen token's logit is within 0.02 + 0.01 |best| of the best."""
    agree = []
    for b, p in enumerate(prompts):
        seq = torch.cat([p, gen[b, :-1]])[None]
        with torch.no_grad():
            lg = m(seq, return_logits=True)["logits"][0, len(p) - 1:].float()
        best = lg.max(-1).values
        got = lg.gather(-1, gen[b][:, None]).squeeze(-1)
        tol = 0.02 + 0.01 * best.abs()
        assert bool((got >= best - tol).all()), (b, (best - got).max().item())
        agree.append((lg.argmax(-1) == gen[b]).float())
    return torch.cat(agree).mean().item()


def _both(m, ids, **kw):
    dev = m.generate(ids, use_graph=True, device_loop=True, **kw)
    host = m.generate(ids, use_graph=True, device_loop=False, **kw)
    assert torch.equal(dev, host), (dev[:, S:].tolist(), host[:, S:].tolist())
    return dev


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_generate_with_mask_end_to_end(name, B):
    m = _model(name)
    prompts, fill = _prompts(m, SEEDS[name])
    prompts = prompts[:B]
    ids, mask = _left(prompts, fill)
    T = 8
    out = _both(m, ids, attention_mask=mask, max_new_tokens=T)
    assert out.shape == (B, S + T) and torch.equal(out[:, :S], ids)
    frac = _judge(m, prompts, out[:, S:])
    print(f"graph: {frac:.2f} of the tokens are the no-cache argmax")
    eager = m.generate(ids, attention_mask=mask.bool(), max_new_tokens=T, use_graph=False)
    assert torch.equal(eager[:, :S], ids)
    _judge(m, prompts, eager[:, S:])
    # sampled: the device loop and the host loop draw the same tokens from the same logits
    kw = dict(attention_mask=mask, max_new_tokens=T, do_sample=True, seed=3, top_k=50, top_p=0.9)
    a = _both(m, ids, **kw)
    assert a.shape == (B, S + T) and torch.equal(a[:, :S], ids)
    assert torch.equal(a, m.generate(ids, **kw))
    assert not torch.equal(a, m.generate(ids, **{**kw, "seed": 4}))


# ------------------------------------------------------------------ 4. device loop
class _OpLog(TorchDispatchMode):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.events.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("name", MODELS)
def test_ragged_device_loop_runs_no_torch_op_between_replays(name, monkeypatch):
    """The logging idiom of test_device_loop_gpu.py::test_no_torch_op_between_replays: every aten op
    the host dispatches is logged from the moment the first replay has returned."""
    from gke_ray_train_amd.models import generation as G
    m = _model(name)
    prompts, fill = _prompts(m, SEEDS[name])
    ids, mask = _left(prompts[:2], fill)
    want = m.generate(ids, attention_mask=mask, max_new_tokens=9, use_graph=True, device_loop=False)
    events, log = [], []
    real = G.GraphDecoder.advance

    def advance(self):
        real(self)
        events.append("replay")
        if not log:
            log.append(_OpLog(events))
            log[0].__enter__()

    monkeypatch.setattr(G.GraphDecoder, "advance", advance)
    try:
        out = m.generate(ids, attention_mask=mask, max_new_tokens=9, use_graph=True)
    finally:
        if log:
            log[0].__exit__(None, None, None)
    assert torch.equal(out, want)
    last = len(events) - 1 - events[::-1].index("replay")
    assert events[:last + 1] == ["replay"] * 8, events  # 9 tokens: the first is eager, then 8 replays
    assert len(events) > last + 1  # the log does see torch ops: the result is assembled afterwards


@pytest.mark.parametrize("name", MODELS)
def test_ragged_early_eos_in_one_row_does_not_stop_the_other(name):
    m = _model(name)
    prompts, fill = _prompts(m, SEEDS[name])
    ids, mask = _left(prompts[:2], fill)
    T = 24
    gen = m.generate(ids, attention_mask=mask, max_new_tokens=T, use_graph=True, device_loop=False)[:, S:].tolist()
    # an id the short row emits within its first 10 tokens and the long row emits later or never
    picks = [(t, tok) for t, tok in enumerate(gen[0][:10]) if tok != 0 and tok not in gen[1][:t + 3]]
    assert picks, "pick another seed: row 1 emits every early token of row 0"
    eos = picks[0][1]
    t0 = gen[0].index(eos)
    out = _both(m, ids, attention_mask=mask, max_new_tokens=T, eos_token_id=eos, pad_token_id=0, sync_every=7)
    t1 = gen[1].index(eos) if eos in gen[1] else T - 1
    assert t1 > t0 and out.shape[1] == S + t1 + 1
    assert torch.equal(out[:, :S], ids)
    assert out[0, S:].tolist() == gen[0][:t0 + 1] + [0] * (t1 - t0)   # pad after its EOS
    assert out[1, S:].tolist() == gen[1][:t1 + 1]                     # the other row is untouched


# ------------------------------------------------------------------ 5. NF4 base + LoRA
def _qlora_model(name, cache, **overrides):
    """As tests/test_nf4_gemv_gpu.py::_qlora_model."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    from gke_ray_train_amd.peft.quant import set_dequant_cache
    m = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=0, **overrides)
    quantize_model_(m, BitsAndBytesConfig())
    if cache is not None:
        set_dequant_cache(m, cache)
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16))
    g = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        for lw in pm.lora_modules.values():
            for p in lw.lora_B.values():
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.05)
    return pm.eval()


def test_qlora_ragged_decode_never_dequantises(monkeypatch):
    from gke_ray_train_amd.models.generation import GraphDecoder, KVCache, forward_cached
    from gke_ray_train_amd.peft.quant import NF4Linear
    pm = _qlora_model("llama-tiny-gqa", "0", intermediate_size=1536)
    model = pm.base_model
    prompts, fill = _prompts(model, 7)
    prompts = prompts[:2]
    ids, mask = _left(prompts, fill)
    T = 8
    dec = GraphDecoder(model, 2, S + T)
    assert dec.norm_ws is None
    logits = dec.prefill(ids, mask)
    cache = KVCache(model.config, 2, S + T, DEV, torch.bfloat16)
    elogits = forward_cached(model, ids, cache, attention_mask=mask)
    count = {"n": 0}
    for name in ("_dequant", "dequantize_into", "_dequant_t"):
        real = getattr(NF4Linear, name)

        def counted(self, *a, _real=real, **k):
            count["n"] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(NF4Linear, name, counted)
    gen, egen = [logits.argmax(-1)], [elogits.argmax(-1)]
    for _ in range(T - 1):
        gen.append(dec.step(gen[-1]).argmax(-1))
    torch.cuda.synchronize()
    assert count["n"] == 0, f"{count['n']} dequantisations in {T - 1} ragged graph decode steps"
    for _ in range(T - 1):
        egen.append(forward_cached(model, egen[-1][:, None], cache).argmax(-1))
    assert count["n"] == 0, f"{count['n']} dequantisations in {T - 1} ragged eager decode steps"
    _judge(pm, prompts, torch.stack(gen, 1))
    _judge(pm, prompts, torch.stack(egen, 1))
    assert count["n"] > 0  # the counters do count: the judge's full forward dequantises
    out = pm.generate(ids, attention_mask=mask, max_new_tokens=T)
    assert torch.equal(out[:, :S], ids) and torch.equal(out[:, S:], torch.stack(gen, 1))


# ------------------------------------------------------------------ 6. pad ids
@pytest.mark.parametrize("name", MODELS)
def test_pad_ids_do_not_matter(name):
    m = _model(name)
    prompts, fill = _prompts(m, SEEDS[name])
    ids, mask = _left(prompts, fill)
    pad_id = 2
    ids_pad, _ = _left(prompts, torch.full_like(fill, pad_id))
    assert not torch.equal(ids, ids_pad)
    for kw in (dict(use_graph=True), dict(use_graph=False)):
        a = m.generate(ids, attention_mask=mask, max_new_tokens=8, pad_token_id=pad_id, **kw)
        b = m.generate(ids_pad, attention_mask=mask, max_new_tokens=8, pad_token_id=pad_id, **kw)
        assert torch.equal(a[:, S:], b[:, S:]), kw
    la = _run("graph", m, ids, mask, None)
    lb = _run("graph", m, ids_pad, mask, la[:-1].argmax(-1))
    _close(lb, la, LOGIT_TOL, LOGIT_TOL, f"{name}: pad columns of pad_token_id vs random ids")
