"""``generate()`` with the token picked inside the captured decode step (``GraphDecoder`` with a
``SamplerConfig``: the device loop) against the host loop on the same graph's logits. Both loops read
the same logits, so every comparison is exact. The no-torch-op check logs every aten op the host
dispatches (a ``TorchDispatchMode``) together with the replays and looks at what lies between them."""
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 12
MODELS = ["llama-tiny-d64", "llama-tiny-gqa"]
_cache = {}


def _model(name):
    from gke_ray_train_amd.models import build_llama
    if name not in _cache:
        _cache[name] = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=0).eval()
    return _cache[name]


def _ids(m, B, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, m.config.vocab_size, (B, S), device=DEV, generator=g)


def _both(m, ids, **kw):
    dev = m.generate(ids, use_graph=True, device_loop=True, **kw)
    host = m.generate(ids, use_graph=True, device_loop=False, **kw)
    assert torch.equal(dev, host), (kw, dev[:, S:].tolist(), host[:, S:].tolist())
    return dev


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", MODELS)
def test_greedy_device_loop_equals_host_loop(name, B):
    m = _model(name)
    ids = _ids(m, B, 4)
    T = 40
    plain = _both(m, ids, max_new_tokens=T)
    assert plain.shape == (B, S + T) and torch.equal(plain[:, :S], ids)
    assert torch.equal(_both(m, ids, max_new_tokens=T, sync_every=7), plain)
    assert torch.equal(_both(m, ids, max_new_tokens=17, sync_every=16), plain[:, :S + 17])
    assert torch.equal(_both(m, ids, max_new_tokens=1), plain[:, :S + 1])
    # an EOS id taken from the greedy output, as tests/test_gpu_jobs.py does
    gen = plain[:, S:].tolist()
    eos = gen[0][5]
    for kw in (dict(), dict(sync_every=7), dict(sync_every=1)):
        out = _both(m, ids, max_new_tokens=T, eos_token_id=eos, pad_token_id=0, **kw)
        stop = max(row.index(eos) if eos in row else T - 1 for row in gen)  # the token that finishes the last row
        assert out.shape[1] == S + stop + 1, (out.shape, stop)
        assert torch.equal(out[0, S:S + gen[0].index(eos) + 1], plain[0, S:S + gen[0].index(eos) + 1])
    # a list of EOS ids, no pad id: finished rows keep emitting their tokens
    _both(m, ids, max_new_tokens=T, eos_token_id=[eos, gen[-1][9], 3], sync_every=5)


@pytest.mark.parametrize("name", MODELS)
def test_one_row_finishes_early_and_the_other_runs_on(name):
    m = _model(name)
    ids = _ids(m, 2, 4)
    T = 32
    gen = m.generate(ids, max_new_tokens=T, use_graph=True, device_loop=False)[:, S:].tolist()
    # an id row 0 emits within its first 10 tokens and row 1 emits later or never
    picks = [(t, tok) for t, tok in enumerate(gen[0][:10]) if tok != 0 and tok not in gen[1][:t + 3]]
    assert picks, "pick another prompt seed: row 1 emits every early token of row 0"
    t0, eos = picks[0]
    t0 = gen[0].index(eos)
    out = _both(m, ids, max_new_tokens=T, eos_token_id=eos, pad_token_id=0, sync_every=7)
    t1 = gen[1].index(eos) if eos in gen[1] else T - 1
    assert t1 > t0 and out.shape[1] == S + t1 + 1
    assert out[0, S:].tolist() == gen[0][:t0 + 1] + [0] * (t1 - t0)   # pad after its EOS
    assert out[1, S:].tolist() == gen[1][:t1 + 1]                     # the other row is untouched


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", MODELS)
def test_sampled_device_loop_equals_host_loop(name, B):
    m = _model(name)
    ids = _ids(m, B, 5)
    kw = dict(max_new_tokens=24, do_sample=True, seed=3, top_k=50, top_p=0.9)
    a = _both(m, ids, **kw)
    assert torch.equal(a, m.generate(ids, use_graph=True, device_loop=True, **kw))  # same seed: identical
    b = m.generate(ids, use_graph=True, device_loop=True, **{**kw, "seed": 4})
    assert not torch.equal(a, b)
    # seed=None: torch's default generator picks it
    torch.manual_seed(9)
    c = m.generate(ids, **{**kw, "seed": None})
    torch.manual_seed(9)
    assert torch.equal(c, m.generate(ids, **{**kw, "seed": None}))


class _OpLog(TorchDispatchMode):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.events.append(str(func))
        return func(*args, **(kwargs or {}))


def _logged_generate(monkeypatch, m, ids, **kw):
    """generate() on the device loop with every aten op the host dispatches logged from the moment
    the first replay (the one that captures) has returned."""
    from gke_ray_train_amd.models import generation as G
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
        out = m.generate(ids, use_graph=True, **kw)
    finally:
        if log:
            log[0].__exit__(None, None, None)
    return out, events


@pytest.mark.parametrize("name", MODELS)
def test_no_torch_op_between_replays(name, monkeypatch):
    m = _model(name)
    ids = _ids(m, 2, 4)
    want = m.generate(ids, max_new_tokens=9, use_graph=True, device_loop=False)
    out, events = _logged_generate(monkeypatch, m, ids, max_new_tokens=9)
    assert torch.equal(out, want)
    last = len(events) - 1 - events[::-1].index("replay")
    assert events[:last + 1] == ["replay"] * 8, events  # 9 tokens: the first is eager, then 8 replays
    assert len(events) > last + 1  # the log does see torch ops: the result is assembled after the last replay
    # with an EOS id the host reads finished.all() every sync_every tokens, and nothing else
    out, events = _logged_generate(monkeypatch, m, ids, max_new_tokens=9, eos_token_id=[511, 510], sync_every=4)
    assert torch.equal(out, want) or out.shape[1] < want.shape[1]
    last = len(events) - 1 - events[::-1].index("replay")
    tokens, between = 1, {}
    for e in events[:last + 1]:
        if e == "replay":
            tokens += 1
        else:
            between.setdefault(tokens, []).append(e)
    assert set(between) <= {4, 8}, between
    for ops in between.values():
        assert any("all" in o for o in ops) and len(ops) <= 3, between


def test_switch_restores_the_host_loop(monkeypatch):
    from gke_ray_train_amd.models import generation as G
    m = _model("llama-tiny-d64")
    ids = _ids(m, 2, 4)
    want = m.generate(ids, max_new_tokens=8, use_graph=True)
    calls = []
    real = G.GraphDecoder.advance
    monkeypatch.setattr(G.GraphDecoder, "advance", lambda self: (calls.append(1), real(self))[1])
    assert torch.equal(m.generate(ids, max_new_tokens=8, use_graph=True), want) and len(calls) == 7
    monkeypatch.setattr(G, "_DEVICE_SAMPLER", False)  # GRT_DEVICE_SAMPLER=0
    assert torch.equal(m.generate(ids, max_new_tokens=8, use_graph=True), want) and len(calls) == 7
    # a caller's generator keeps torch.multinomial's path; 9 EOS ids do not fit the kernel's list
    monkeypatch.setattr(G, "_DEVICE_SAMPLER", True)
    g = torch.Generator(device=DEV).manual_seed(1)
    m.generate(ids, max_new_tokens=4, use_graph=True, do_sample=True, top_p=0.9, top_k=20, generator=g)
    m.generate(ids, max_new_tokens=4, use_graph=True, eos_token_id=list(range(100, 109)))
    assert len(calls) == 7
    with pytest.raises(ValueError, match="device_loop"):
        m.generate(ids, max_new_tokens=4, use_graph=True, eos_token_id=list(range(100, 109)), device_loop=True)
    # the decoder's two interfaces do not mix
    dec = G.GraphDecoder(m, 2, 32)
    with pytest.raises(RuntimeError, match="SamplerConfig"):
        dec.advance()
    dec = G.GraphDecoder(m, 2, 32, sampler=G.SamplerConfig(max_new_tokens=4))
    with pytest.raises(RuntimeError, match="advance"):
        dec.step(ids[:, 0])


def test_lora_nf4_model_generates_through_the_device_loop():
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    m = build_llama("llama-tiny-gqa", device=DEV, dtype=torch.bfloat16, seed=0, intermediate_size=1536)
    quantize_model_(m, BitsAndBytesConfig())
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16))
    g = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        for lw in pm.lora_modules.values():
            for p in lw.lora_B.values():
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.05)
    pm.eval()
    ids = torch.randint(0, 512, (2, S), device=DEV, generator=g)
    out = _both(pm, ids, max_new_tokens=16)
    assert out.shape == (2, S + 16)
    _both(pm, ids, max_new_tokens=16, do_sample=True, seed=3, top_k=50, top_p=0.9)
