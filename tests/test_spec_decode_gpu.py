"""Prompt-lookup speculative decoding on the GPU: the multi-token decode attention kernel
(decode_attention.hip), the sampler's candidate mode (sample.hip), the accept + draft kernel
(spec.hip), the verify step of ``GraphDecoder`` and ``generate(..., prompt_lookup_num_tokens=K)``.

Bounds: attention against the fp32 math of ``ops/_ref.py`` at 1e-2 absolute and relative
(tests/test_decode_d64_gpu.py); the integer kernels bitwise against their host implementations;
verify-step logits against the one-token ``GraphDecoder`` at ``LOGIT_TOL`` with argmax equality on
decisive steps, end-to-end tokens by ``_judge`` (both rules are tests/test_ragged_generate_gpu.py's).
Model seeds are chosen from the plain one-token runs alone."""
import math

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

DEV = "cuda"
QNAN = 0x7FC00000
LOGIT_TOL = 2e-2
S = 12
NEW = 17          # new tokens of the end-to-end runs: not a multiple of K + 1 for K = 1, 3
MODELS = ["llama-tiny-gqa", "llama-tiny-d64"]
_cache = {}


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


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


# ------------------------------------------------------------------ 1. attn_decode_multi
CACHE = 600


def _multi(D):
    return _C().attn_decode_multi if D == 128 else _C().attn_decode_multi_d64


def _single(D):
    return _C().attn_decode if D == 128 else _C().attn_decode_d64


def _qkv(B, T, G, D, seed):
    """q [B, T, 2 G, D] and a STRIDED cache view k / v [B, CACHE, 2, D] (longer rows, wider heads)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, T, 2 * G, D, device=DEV, dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, CACHE + 20, 2, D + 8, device=DEV, dtype=torch.bfloat16, generator=g)[:, :CACHE, :, :D]
    v = torch.randn(B, CACHE + 20, 2, D + 8, device=DEV, dtype=torch.bfloat16, generator=g)[:, :CACHE, :, :D]
    assert not k.is_contiguous()
    return q, k, v


def _check_multi(q, k, v, lens, what):
    """The kernel against the fp32 math and against the one-token kernel, token by token."""
    from gke_ray_train_amd.ops import _ref
    B, T, _, D = q.shape
    sl = None if lens is None else torch.tensor(lens, device=DEV, dtype=torch.int32)
    full = torch.full((B,), k.shape[1], device=DEV, dtype=torch.int32) if sl is None else sl
    o = _multi(D)(q, k, v, sl, D ** -0.5)
    assert o.shape == q.shape and o.dtype == torch.bfloat16 and o.is_contiguous()
    for t in range(T):
        len_t = full - (T - 1 - t)
        ref = _ref.attention(q[:, t:t + 1].float(), k.float(), v.float(), causal=False, seqlens_k=len_t)
        _close(o[:, t:t + 1], ref, 1e-2, 1e-2, f"{what} token {t} vs fp32 math")
        one = _single(D)(q[:, t:t + 1], k, v, len_t, D ** -0.5)
        _close(o[:, t:t + 1], one, 1e-2, 1e-2, f"{what} token {t} vs attn_decode")
        dead = len_t <= 0
        if bool(dead.any()):  # a token with no key: output 0
            assert not o[:, t][dead].float().abs().any()


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_multi_matches_fp32_math_and_the_one_token_kernel(D, G, T):
    """Valid lengths T (every token sees 1 .. T keys), 17, 256 / 257 and 333 in a cache of 600 slots
    (333 leaves the trailing splits empty); B = 2 with unequal lengths, one of them shorter than T
    (its first tokens have no key at all); cache views of 256 and 257 slots, which at head_dim 64
    lie on either side of the one-launch threshold. G = 8 with T = 4 tiles the tokens over the grid."""
    q, k, v = _qkv(1, T, G, D, 10 * G + T)
    for n in (T, 17, 256, 257, 333):
        _check_multi(q, k, v, [n], f"D={D} G={G} T={T} B=1 len={n}")
    for Sk in (256, 257):
        _check_multi(q, k[:, :Sk], v[:, :Sk], None, f"D={D} G={G} T={T} B=1 cache={Sk}")
        _check_multi(q, k[:, :Sk], v[:, :Sk], [Sk - 3], f"D={D} G={G} T={T} B=1 cache={Sk} len={Sk - 3}")
    q, k, v = _qkv(2, T, G, D, 20 * G + T)
    for lens in ([257, 17], [T, 333], [T - 1, 256]):
        _check_multi(q, k, v, lens, f"D={D} G={G} T={T} B=2 lens={lens}")
    _check_multi(q, k[:, :200], v[:, :200], [200, 31], f"D={D} G={G} T={T} B=2 cache=200")


@pytest.mark.parametrize("D,Sk", [(64, 200), (64, 333), (128, 333)])  # one launch; split + combine
def test_attn_decode_multi_reads_no_stale_lds(D, Sk):
    C = _C()
    q, k, v = _qkv(2, 4, 4, D, 7)
    k, v = k[:, :Sk], v[:, :Sk]
    sl = torch.tensor([Sk, 90], device=DEV, dtype=torch.int32)
    dev = torch.cuda.current_device()
    outs = []
    for pattern in (QNAN, 0):
        C.lds_fill(pattern, dev)
        outs.append(_multi(D)(q, k, v, sl, D ** -0.5))
    assert torch.isfinite(outs[0].float()).all() and torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(_multi(D)(q, k, v, sl, D ** -0.5), _multi(D)(q, k, v, sl, D ** -0.5))


def test_attn_decode_multi_refusals():
    """Every refused call's operands lie inside live allocations."""
    from gke_ray_train_amd import ops
    C = _C()
    q, k, v = _qkv(2, 4, 2, 64, 1)
    assert C.attn_decode_multi_d64(q, k, v, None, 0.125).shape == q.shape  # the accepted baseline
    q5 = torch.randn(2, 5, 4, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="2 to 4 query tokens"):
        C.attn_decode_multi_d64(q5, k, v, None, 0.125)
    with pytest.raises(RuntimeError, match="2 to 4 query tokens"):
        C.attn_decode_multi_d64(q[:, :1], k, v, None, 0.125)
    with pytest.raises(RuntimeError, match="bf16"):
        C.attn_decode_multi_d64(q.float(), k.float(), v.float(), None, 0.125)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        C.attn_decode_multi(q, k, v, None, 0.125)
    q32 = torch.randn(2, 4, 4, 32, device=DEV, dtype=torch.bfloat16)
    kv32 = torch.randn(2, 16, 2, 32, device=DEV, dtype=torch.bfloat16)
    with pytest.raises((RuntimeError, ValueError), match="head_dim"):
        ops.decode_attention_multi(q32, kv32, kv32)
    q6 = torch.randn(2, 4, 6, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GQA group"):
        C.attn_decode_multi_d64(q6, k, v, None, 0.125)


# ------------------------------------------------------------------ 2. draft kernel
def _state(K, n=0, max_new=8, prompt_len=0, hist=None, drafts=None, cand=None, finished=False, pos0=0):
    """Device state of one spec_advance call, as GraphDecoder keeps it."""
    T = K + 1
    st = dict(
        cand=torch.tensor(cand if cand is not None else [0] * T, device=DEV),
        drafts=torch.tensor(drafts if drafts is not None else [-1] * K, device=DEV),
        ids=torch.full((T,), 99, device=DEV),
        pos=torch.arange(pos0, pos0 + T, device=DEV, dtype=torch.int32),
        lens=torch.tensor([pos0 + T], device=DEV, dtype=torch.int32),
        n_step=torch.tensor([n], device=DEV), counter=torch.tensor([n], device=DEV),
        finished=torch.tensor([finished], device=DEV), finish_step=torch.tensor([-1], device=DEV),
        done=torch.zeros(1, dtype=torch.bool, device=DEV),
        out=torch.full((max_new,), -7, device=DEV),
        hist=torch.full((prompt_len + max_new,), -7, device=DEV))
    if hist is not None:
        st["hist"][:len(hist)] = torch.tensor(hist, device=DEV)
    return st


def _advance(st, prompt_len, max_new, N, vocab=512, plan=None, eos=None):
    _C().spec_advance(st["cand"], st["drafts"], st["ids"], st["pos"], st["lens"], st["n_step"], st["counter"],
                      st["finished"], st["finish_step"], st["done"], st["out"], st["hist"], prompt_len, max_new, N, vocab,
                      plan=plan, eos_ids=None if eos is None else torch.tensor(eos, device=DEV))


@pytest.mark.parametrize("n_hist", [1, 2, 5, 1500])
def test_draft_kernel_matches_the_host_lookup(n_hist):
    """Random histories over 4 ids. The history reaches the kernel as a prompt of n_hist - 1
    tokens plus the one token the step emits; 1500 tokens are more than one loop trip per thread."""
    from gke_ray_train_amd.ops import _ref
    g = torch.Generator().manual_seed(n_hist)
    for trial in range(3):
        h = torch.randint(0, 4, (n_hist,), generator=g).tolist()
        for K in (1, 2, 3):
            for N in (1, 2, 3, 4):
                st = _state(K, max_new=4, prompt_len=n_hist - 1, hist=h[:-1], cand=[h[-1]] * (K + 1))
                _advance(st, n_hist - 1, 4, N)
                want = _ref.prompt_lookup_draft(h, n_hist, K, N)
                assert st["hist"][:n_hist].tolist() == h
                assert st["drafts"].tolist() == want, (h[-12:], K, N)
                assert st["ids"].tolist() == [h[-1]] + [max(d, 0) for d in want]


def test_draft_kernel_plan_path():
    plan = torch.tensor([11, 12, 13, 14, 600, 16], device=DEV)
    for K in (1, 2, 3):
        for n in (0, 2, 4):
            st = _state(K, n=n, max_new=9, prompt_len=3, hist=[1, 2, 1], cand=[5] * (K + 1))
            _advance(st, 3, 9, 2, plan=plan)
            want = (plan.tolist()[n + 1:n + 1 + K] + [-1] * K)[:K]   # one token was emitted: n' = n + 1
            assert st["drafts"].tolist() == want
            # an id outside the vocabulary (600) stays in `drafts` and embeds as id 0
            assert st["ids"].tolist() == [5] + [d if 0 <= d < 512 else 0 for d in want]


# ------------------------------------------------------------------ 3. candidate mode
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [512, 517])
def test_candidate_mode_matches_the_host_sampler_row_by_row(V, dtype):
    from gke_ray_train_amd.ops import _ref
    g = torch.Generator(device=DEV).manual_seed(V)
    logits = (torch.randn(4, V, device=DEV, generator=g) * 3).to(dtype)
    counter = torch.tensor([5], device=DEV)
    for kw in (dict(do_sample=False), dict(do_sample=True, seed=3, top_k=50, top_p=0.9, temperature=0.8),
               dict(do_sample=True, seed=4)):
        cand = torch.full((4,), -1, device=DEV)
        got = _C().sample_logits(logits, counter=counter, next_ids=cand, candidates=True, **kw)
        assert got.data_ptr() == cand.data_ptr() and int(counter) == 5
        want = [int(_ref.sample_tokens(logits[t:t + 1], counter=5 + t, **kw)) for t in range(4)]
        assert cand.tolist() == want, kw
        # and it is what the one-row kernel call draws at that token number
        one = [int(_C().sample_logits(logits[t:t + 1], counter=torch.tensor([5 + t], device=DEV), **kw)) for t in range(4)]
        assert one == want, kw
    with pytest.raises(RuntimeError, match="candidates"):
        z = torch.zeros(4, dtype=torch.long, device=DEV)
        _C().sample_logits(logits, candidates=True, finished=torch.zeros(4, dtype=torch.bool, device=DEV),
                           finish_step=z, step=z[:1], out=z.view(4, 1).clone())


# ------------------------------------------------------------------ 4. spec_advance
ACCEPT_CASES = [
    # drafts, cand, n, max_new, eos, finished
    ([4, 5, 6], [4, 5, 6, 7], 2, 100, (), False),        # all accepted
    ([4, 5, 6], [9, 5, 6, 7], 2, 100, (), False),        # first draft rejected
    ([4, 5, 6], [4, 8, 6, 7], 2, 100, (), False),
    ([4, -1, -1], [4, 5, 6, 7], 0, 100, (), False),      # an open slot
    ([-1, -1, -1], [4, 5, 6, 7], 0, 100, (), False),
    ([4, 5, 6], [4, 5, 6, 7], 10, 100, (5,), False),     # EOS in the middle of an accepted run
    ([4, 5, 6], [4, 5, 6, 7], 10, 100, (4, 7), False),
    ([4, 5, 6], [4, 5, 6, 7], 6, 8, (), False),          # cut at max_new_tokens
    ([4, 5, 6], [4, 5, 6, 7], 7, 8, (5,), False),
    ([4, 5, 6], [4, 5, 6, 7], 3, 100, (), True),         # finished: inert
    ([4, 5, 6], [4, 5, 6, 7], 8, 8, (), False),          # full: inert
    ([4, 5], [4, 5, 6], 1, 100, (), False),              # K = 2
    ([4], [9, 5], 1, 100, (9,), False),                  # K = 1
]


@pytest.mark.parametrize("case", range(len(ACCEPT_CASES)))
def test_spec_advance_matches_the_host_accept_step(case):
    from gke_ray_train_amd.ops import _ref
    drafts, cand, n, max_new, eos, finished = ACCEPT_CASES[case]
    K, P, pos0 = len(drafts), 3, 3 + n - 1
    emitted, fin, fstep = _ref.spec_accept(drafts, cand, n, max_new, eos, finished)
    st = _state(K, n=n, max_new=max_new, prompt_len=P, hist=[1, 2, 1], drafts=drafts, cand=cand, finished=finished,
                pos0=pos0)
    before = {k: v.clone() for k, v in st.items()}
    _advance(st, P, max_new, 2, eos=list(eos) or None)
    e = len(emitted)
    if e == 0:  # inert: nothing at all changes
        for k in st:
            assert torch.equal(st[k], before[k]), k
        return
    assert st["out"][n:n + e].tolist() == emitted and st["hist"][P + n:P + n + e].tolist() == emitted
    assert torch.equal(st["out"][n + e:], before["out"][n + e:]) and torch.equal(st["out"][:n], before["out"][:n])
    assert int(st["n_step"]) == n + e and int(st["counter"]) == n + e
    assert bool(st["finished"]) == fin and int(st["finish_step"]) == fstep
    assert int(st["ids"][0]) == emitted[-1]
    assert st["pos"].tolist() == [pos0 + e + t for t in range(K + 1)] and int(st["lens"]) == pos0 + e + K + 1
    assert bool(st["done"]) == (fin or n + e >= max_new)
    # a finished or full row: one more call changes nothing
    if bool(st["done"]):
        after = {k: v.clone() for k, v in st.items()}
        _advance(st, P, max_new, 2, eos=list(eos) or None)
        for k in st:
            assert torch.equal(st[k], after[k]), k


# ------------------------------------------------------------------ 5. verify-step logits
def _eos_picks(gen, agree):
    """Token numbers of a plain run that can serve as an EOS inside an accepted K = 3 run: i with
    (i - 1) % 4 != 3 is not the last token of its verify step, so with the plain run as the plan
    the drafts after it are right as well and only the EOS cuts them off. The token must not occur
    earlier, and it and its successor lie before the first non-decisive step."""
    return [i for i in range(1, min(agree, NEW) - 1) if (i - 1) % 4 != 3 and gen[i] not in gen[:i]]


def _plain(name):
    """The plain one-token ``GraphDecoder`` run (greedy, NEW tokens) of one model seed of 0-31,
    chosen from the plain runs alone: decisive steps are those whose reference top-1 / top-2 margin
    is over twice the logit tolerance, and the seed taken is one whose run offers an EOS token
    (``_eos_picks``), with the longest decisive prefix and then the most decisive steps. Returns
    (model, ids, tokens [NEW], logits [NEW, V], decisive [NEW] bool); logits[i] are those token i
    was picked from."""
    if ("plain", name) in _cache:
        return _cache["plain", name]
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models import generation as G
    best, best_score = None, None
    for seed in range(32):
        m = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=seed).eval()
        ids = torch.randint(0, m.config.vocab_size, (1, S), device=DEV,
                            generator=torch.Generator(device=DEV).manual_seed(seed))
        dec = G.GraphDecoder(m, 1, S + NEW)
        lg = [dec.prefill(ids).clone()]
        for _ in range(NEW - 1):
            lg.append(dec.step(lg[-1].argmax(-1)).clone())
        lg = torch.cat(lg)
        top2 = lg.topk(2, -1).values
        decisive = (top2[:, 0] - top2[:, 1]) > 2 * (LOGIT_TOL + LOGIT_TOL * top2[:, 0].abs())
        toks = lg.argmax(-1)
        agree = _first_open(decisive)
        score = (bool(_eos_picks(toks.tolist(), agree)), agree, int(decisive.sum()))
        if best is None or score > best_score:
            best, best_score = (m, ids, toks, lg, decisive), score
    print(f"{name}: {int(best[4].sum())} of {NEW} plain steps are decisive, the first {best_score[1]} in a row")
    assert best[4].float().mean().item() >= 0.5, "no seed in 0-31 with decisive greedy steps"
    _cache["plain", name] = best
    return best


def _first_open(decisive):
    """Index of the first non-decisive step (NEW if none): tokens before it must be the plain run's."""
    bad = (~decisive).nonzero()
    return int(bad[0]) if len(bad) else NEW


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_verify_step_logits_match_the_one_token_decoder(name, K):
    from gke_ray_train_amd.models import generation as G
    m, ids, toks, ref, decisive = _plain(name)
    T = K + 1
    dec = G.GraphDecoder(m, 1, S + NEW + K, spec=G.SpecConfig(K))
    assert dec.norm_ws is None
    first = dec.prefill(ids)
    _close(first, ref[:1], LOGIT_TOL, LOGIT_TOL, f"{name}: prefill")
    n = 1
    while n + T <= NEW:  # inputs: token n - 1 and the plain run's next K tokens, at positions S + n - 1 ...
        lg = dec.step_spec(toks[n - 1:n + K], S + n - 1)
        _close(lg, ref[n:n + T], LOGIT_TOL, LOGIT_TOL, f"{name} K={K}: verify step at token {n}")
        d = decisive[n:n + T]
        assert torch.equal(lg.argmax(-1)[d], toks[n:n + T][d])
        n += T
    assert dec.n_replays == (NEW - 1) // T


# ------------------------------------------------------------------ 6. generate() end to end
def _judge(m, prompt, gen):
    """test_ragged_generate_gpu.py's rule: each generated token against a no-cache forward over
    the prefix: the chosen token's logit is within 0.02 + 0.01 |best| of the best."""
    seq = torch.cat([prompt, gen[:-1]])[None]
    with torch.no_grad():
        lg = m(seq, return_logits=True)["logits"][0, len(prompt) - 1:].float()
    best = lg.max(-1).values
    got = lg.gather(-1, gen[:, None]).squeeze(-1)
    tol = 0.02 + 0.01 * best.abs()
    assert bool((got >= best - tol).all()), (best - got).max().item()


def _both(m, ids, **kw):
    from gke_ray_train_amd.models import generation as G
    dev = m.generate(ids, use_graph=True, device_loop=True, **kw)
    stats = dict(G.last_spec_stats)
    host = m.generate(ids, use_graph=True, device_loop=False, **kw)
    assert torch.equal(dev, host), (dev[:, ids.shape[1]:].tolist(), host[:, ids.shape[1]:].tolist())
    return dev, stats


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_generate_greedy_end_to_end(name, K):
    m, ids, toks, _, decisive = _plain(name)
    plain = m.generate(ids, max_new_tokens=NEW, use_graph=True, device_loop=True)
    assert plain.shape == (1, S + NEW)
    agree = _first_open(decisive)
    # the plain run as the plan: every draft is right wherever the two decoders agree
    out, stats = _both(m, ids, max_new_tokens=NEW, prompt_lookup_num_tokens=K, _spec_plan=plain[0, S:].clone())
    assert out.shape == (1, S + NEW) and torch.equal(out[:, :S], ids)   # NEW is no multiple of K + 1
    _judge(m, ids[0], out[0, S:])
    assert torch.equal(out[0, S:S + agree], plain[0, S:S + agree])
    assert stats["n_emitted"] == NEW
    bound = math.ceil((NEW - 1) / (K + 1)) + int((~decisive).sum())
    # generate() replays on until a host read sees the done flag: read it after every replay
    from gke_ray_train_amd.models import generation as G
    again = m.generate(ids, max_new_tokens=NEW, use_graph=True, device_loop=True, prompt_lookup_num_tokens=K,
                       _spec_plan=plain[0, S:].clone(), sync_every=1)
    assert torch.equal(again, out)
    print(f"{name} K={K}: {G.last_spec_stats}, bound {bound}")
    assert G.last_spec_stats["n_replays"] <= bound, (G.last_spec_stats, bound)
    # a plan that is wrong at two token numbers, and the real lookup: still the plain tokens
    bad = plain[0, S:].clone()
    bad[3] = (bad[3] + 1) % 512
    bad[9] = (bad[9] + 1) % 512
    for kw in (dict(_spec_plan=bad), dict(max_matching_ngram_size=2)):
        out, _ = _both(m, ids, max_new_tokens=NEW, prompt_lookup_num_tokens=K, **kw)
        assert out.shape == (1, S + NEW)
        _judge(m, ids[0], out[0, S:])
        assert torch.equal(out[0, S:S + agree], plain[0, S:S + agree]), kw


@pytest.mark.parametrize("name", MODELS)
def test_generate_real_lookup_on_a_repetitive_prompt(name):
    """A prompt over 4 ids: the lookup drafts at every step. Both loops, judged token by token."""
    m, _, _, _, _ = _plain(name)
    ids = torch.randint(0, 4, (1, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out, stats = _both(m, ids, max_new_tokens=NEW, prompt_lookup_num_tokens=3)
    assert out.shape == (1, 40 + NEW)
    _judge(m, ids[0], out[0, 40:])
    print(f"{name}: {stats}")


@pytest.mark.parametrize("name", MODELS)
def test_generate_sampled_device_loop_equals_host_loop(name):
    m, ids, _, _, _ = _plain(name)
    kw = dict(max_new_tokens=NEW, do_sample=True, seed=3, top_k=50, top_p=0.9, prompt_lookup_num_tokens=3)
    plain = m.generate(ids, use_graph=True, **{**kw, "prompt_lookup_num_tokens": None})
    a, _ = _both(m, ids, _spec_plan=plain[0, S:].clone(), **kw)
    assert a.shape == (1, S + NEW)
    b, _ = _both(m, ids, **kw)
    assert b.shape == (1, S + NEW)
    c = m.generate(ids, use_graph=True, _spec_plan=plain[0, S:].clone(), **{**kw, "seed": 4})
    assert not torch.equal(a, c)


def _sampled_plain(m, ids, seed):
    """The plain run with temperature-1 sampling (no top-k / top-p: every token is kept), by the
    one-token ``GraphDecoder`` and the sampler's host implementation. A step is decisive when the
    best and the second best of logit + noise are further apart than twice the logit tolerance at
    the largest logit of the row: then no error within the tolerance changes the draw."""
    from gke_ray_train_amd.models import generation as G
    from gke_ray_train_amd.ops import _ref
    dec = G.GraphDecoder(m, 1, S + NEW)
    lg = dec.prefill(ids)
    toks, decisive = [], []
    for t in range(NEW):
        score = lg.double() + _ref.sample_noise(seed, t, 1, lg.shape[1], DEV)
        top2 = score[0].topk(2).values
        decisive.append(float(top2[0] - top2[1]) > 2 * (LOGIT_TOL + LOGIT_TOL * float(lg.abs().max())))
        toks.append(int(_ref.sample_tokens(lg, seed=seed, counter=t)))
        if t + 1 < NEW:
            lg = dec.step(torch.tensor([toks[-1]], device=DEV))
    return toks, torch.tensor(decisive)


@pytest.mark.parametrize("name", MODELS)
def test_generate_stops_right_after_an_eos_inside_an_accepted_run(name):
    """Sampled, because a random-init model's greedy run repeats one token wherever its steps are
    decisive, and an EOS must be a token's first occurrence. The sampling seed is the first of 0-15
    whose plain run (alone) offers an EOS (``_eos_picks``)."""
    m, ids, _, _, _ = _plain(name)
    for seed in range(16):
        gen, decisive = _sampled_plain(m, ids, seed)
        picks = _eos_picks(gen, _first_open(decisive))
        if picks:
            break
    assert picks, "no token of a plain sampled run can serve as the EOS: pick other seeds"
    i = picks[0]
    kw = dict(max_new_tokens=NEW, use_graph=True, do_sample=True, seed=seed, eos_token_id=gen[i], pad_token_id=0)
    plan = torch.tensor(gen, device=DEV)
    want = m.generate(ids, **kw)
    assert want[0, S:].tolist() == gen[:i + 1]
    for sync in (16, 1):
        out, stats = _both(m, ids, prompt_lookup_num_tokens=3, _spec_plan=plan, sync_every=sync,
                           **{k: v for k, v in kw.items() if k != "use_graph"})
        assert torch.equal(out, want)
        assert stats["n_emitted"] == i + 1
    # greedy: the plain run's token 1 ends the row although the drafts after it are right as well
    _, _, toks, _, _ = _plain(name)
    eos = int(toks[1])
    want = m.generate(ids, max_new_tokens=NEW, use_graph=True, eos_token_id=eos)
    out, _ = _both(m, ids, max_new_tokens=NEW, eos_token_id=eos, prompt_lookup_num_tokens=3, _spec_plan=toks.clone())
    assert torch.equal(out, want) and out.shape[1] <= S + 2


@pytest.mark.parametrize("name", MODELS)
def test_generate_single_padded_row(name):
    m, ids, _, _, _ = _plain(name)
    kw = dict(max_new_tokens=NEW, prompt_lookup_num_tokens=3, use_graph=True)
    want = m.generate(ids, **kw)
    pad = torch.cat([torch.full((1, 5), 3, device=DEV), ids], 1)
    mask = torch.cat([torch.zeros(1, 5, device=DEV), torch.ones(1, S, device=DEV)], 1).long()
    for loop in (True, False):
        out = m.generate(pad, attention_mask=mask, device_loop=loop, **kw)
        assert torch.equal(out[:, :S + 5], pad) and torch.equal(out[:, S + 5:], want[:, S:])


def test_generate_eager_gpu_path():
    m, ids, _, _, decisive = _plain(MODELS[0])
    plain = m.generate(ids, max_new_tokens=NEW, use_graph=False)
    out = m.generate(ids, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=3,
                     _spec_plan=plain[0, S:].clone())
    assert out.shape == (1, S + NEW)
    _judge(m, ids[0], out[0, S:])
    with pytest.raises(ValueError, match=r"1\.\.3"):
        m.generate(ids, max_new_tokens=4, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match="batch of 1"):
        m.generate(ids.repeat(2, 1), max_new_tokens=4, prompt_lookup_num_tokens=2)


class _OpLog(TorchDispatchMode):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.events.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("name", MODELS)
def test_no_torch_op_between_replays(name, monkeypatch):
    """The logging idiom of test_device_loop_gpu.py::test_no_torch_op_between_replays: every aten op
    the host dispatches is logged from the moment the first replay has returned."""
    from gke_ray_train_amd.models import generation as G
    m, ids, _, _, _ = _plain(name)
    kw = dict(max_new_tokens=9, use_graph=True, prompt_lookup_num_tokens=3)
    want = m.generate(ids, device_loop=False, **kw)
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
        out = m.generate(ids, **kw)
    finally:
        if log:
            log[0].__exit__(None, None, None)
    assert torch.equal(out, want)
    last = len(events) - 1 - events[::-1].index("replay")
    assert events[:last + 1] == ["replay"] * 8, events  # at most max_new_tokens - 1 replays, nothing between
    assert len(events) > last + 1  # the log does see torch ops: the result is assembled afterwards
    # with sync_every = 3 the host reads the one done flag between chunks, and nothing else
    events.clear()
    log.clear()
    try:
        out = m.generate(ids, sync_every=3, **kw)
    finally:
        if log:
            log[0].__exit__(None, None, None)
    assert torch.equal(out, want)
    last = len(events) - 1 - events[::-1].index("replay")
    replays, between = 0, {}
    for e in events[:last + 1]:
        if e == "replay":
            replays += 1
        else:
            between.setdefault(replays, []).append(e)
    assert set(between) <= {3, 6}, between
    for ops in between.values():  # bool(done): the scalar read and nothing that launches a kernel
        assert len(ops) <= 2 and all("_local_scalar_dense" in o or "is_nonzero" in o for o in ops), between


# ------------------------------------------------------------------ 7. NF4 base + LoRA
def test_qlora_verify_step_never_dequantises(monkeypatch):
    """As tests/test_ragged_generate_gpu.py::test_qlora_ragged_decode_never_dequantises, with the
    4-row verify step: the NF4 GEMV takes 1-4 rows."""
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.models.generation import GraphDecoder, KVCache, SpecConfig, forward_cached
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    from gke_ray_train_amd.peft.quant import NF4Linear, set_dequant_cache
    m = build_llama("llama-tiny-gqa", device=DEV, dtype=torch.bfloat16, seed=0, intermediate_size=1536)
    quantize_model_(m, BitsAndBytesConfig())
    set_dequant_cache(m, "0")
    pm = get_peft_model(m, LoraConfig(r=8, lora_alpha=16))
    g = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        for lw in pm.lora_modules.values():
            for p in lw.lora_B.values():
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * 0.05)
    pm.eval()
    model = pm.base_model
    ids = torch.randint(0, 512, (1, S), device=DEV, generator=g)
    T = 8
    dec = GraphDecoder(model, 1, S + T + 3, spec=SpecConfig(3))
    dec.prefill(ids)
    cache = KVCache(model.config, 1, S + T + 3, DEV, torch.bfloat16)
    forward_cached(model, ids, cache)
    count = {"n": 0}
    for name in ("_dequant", "dequantize_into", "_dequant_t"):
        real = getattr(NF4Linear, name)

        def counted(self, *a, _real=real, **k):
            count["n"] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(NF4Linear, name, counted)
    step_ids = torch.randint(0, 512, (4,), device=DEV, generator=g)
    graph_lg = [dec.step_spec(step_ids, S + i).clone() for i in range(2)]
    torch.cuda.synchronize()
    assert count["n"] == 0, f"{count['n']} dequantisations in 2 graph verify steps"
    eager_lg = []
    for i in range(2):
        cache.len = S + i
        eager_lg.append(forward_cached(model, step_ids[None], cache, all_logits=True)[0])
    assert count["n"] == 0, f"{count['n']} dequantisations in 2 eager verify steps"
    _close(torch.stack(graph_lg), torch.stack(eager_lg), LOGIT_TOL, LOGIT_TOL, "NF4 + LoRA verify step: graph vs eager")
    out = pm.generate(ids, max_new_tokens=T, prompt_lookup_num_tokens=3)
    assert out.shape == (1, S + T)
    _judge(pm, ids[0], out[0, S:])
    assert count["n"] > 0  # the counters do count: the judge's full forward dequantises
