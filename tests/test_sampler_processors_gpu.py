"""The sampler's logits processors (sample.hip) against ``ops/_ref.py`` on the CPU: exact with top_p = 1, with top-p the
1e-5 band of tests/test_sampler_gpu.py capped at 1 % of the row; ``seen_tokens_add``; ``generate`` on every decode path."""
import math

import pytest
import torch

from gke_ray_train_amd import _native
from gke_ray_train_amd.ops import _ref

pytestmark = pytest.mark.gpu
DEV, LOGIT_TOL, NEW = "cuda", 2e-2, 12


@pytest.mark.parametrize("theta", [1.3, 0.7])
@pytest.mark.parametrize("V", [33, 1000, 4099, 262147])  # the last one reads the bitmap from global memory
def test_kernel_matches_ref(V, theta):
    B, C = 3, _native.kernels()
    g = torch.Generator().manual_seed(V)
    lg = (torch.randn(B, V, generator=g) * 2).bfloat16().float()
    seen = torch.rand(B, V, generator=g) < 0.2
    seen[:, [0, 1, 2, 3, 31, 32, V - 1]] = True
    seen[:, [4, 5]] = False
    # seen: positive, -0, -inf, NaN, negative, +0 and the row's maximum; unseen: the runner-up, an EOS, and 11.5
    lg[:, [0, 1, 2, 3, 31, 32, 4, 5]] = torch.tensor([2.5, -0.0, -math.inf, math.nan, -1.5, 0.0, 11.5, 12.0])
    lg[:, V - 1] = 14.0
    words = _ref.seen_from_bool(seen)
    words[:, (V - 1) >> 5] |= -2 ** 31  # the last bit of the last word: a bit past V (no V here is a multiple of 32)
    eos, fin = [5, 6], torch.tensor([False, True, False])
    for dtype in (torch.float32, torch.bfloat16):
        buf = torch.full((B, V + 3), 1e30, dtype=dtype, device=DEV)  # padded stride: misaligned rows
        buf[:, :V] = lg
        for kw in (dict(), dict(do_sample=True, temperature=0.8, min_p=0.05, seed=V),
                   dict(do_sample=True, temperature=0.8, min_p=0.05, top_k=20, top_p=0.9, seed=V)):
            ref_kw = {k: v for k, v in kw.items() if k != "seed"}
            want = _ref.sample_tokens(lg, seed=V, repetition_penalty=theta, seen=seen, suppress=eos,
                                      **{"do_sample": False, **ref_kw})
            ref_kw.pop("do_sample", None)
            _, keep, frac = _ref.sample_filter(lg, repetition_penalty=theta, seen=seen, suppress=eos, **ref_kw)
            band = ((frac - kw.get("top_p", 2.0)).abs() <= 1e-5) & (frac > 0)  # empty without top-p
            assert int(band.sum(-1).max()) <= 0.01 * V
            mask = torch.full((B, V), 7, dtype=torch.uint8, device=DEV) if kw else None
            bitmap, out = words.to(DEV), torch.zeros(B, 4, dtype=torch.long, device=DEV)
            tok = C.sample_logits(buf[:, :V], keep_mask=mask, seen=bitmap, repetition_penalty=theta, min_new_tokens=2,
                                  finished=fin.to(DEV), finish_step=torch.zeros(B, dtype=torch.long, device=DEV),
                                  step=torch.ones(1, dtype=torch.long, device=DEV), out=out,
                                  eos_ids=torch.tensor(eos, device=DEV), pad_id=7, max_steps=4, **kw).cpu()
            if kw:
                assert torch.equal(mask.cpu().bool() | band, keep | band), (V, theta, dtype, kw)
            else:  # 14 / 1.3 < 11.5 and the 12 is a suppressed EOS; 14 / 0.7 stays on top
                assert want.tolist() == [4 if theta > 1 else V - 1] * B
            assert torch.equal(tok, torch.where(fin, torch.tensor(7), want)), (V, theta, dtype, kw, tok, want)
            bit = torch.zeros(B, V, dtype=torch.bool).scatter_(1, want[:, None], ~fin[:, None])
            assert torch.equal(bitmap.cpu(), words | _ref.seen_from_bool(bit))


def test_seen_tokens_add():
    B, S, V = 3, 30000, 1000  # B * S ids: more than one trip of the 256 x 256 thread grid
    ids = torch.randint(-1, V + 1, (B, S + 5), generator=torch.Generator().manual_seed(0))[:, :S]  # -1, V, duplicates
    for lens in (None, [0, 17, S]):
        n = torch.tensor(lens or [S] * B)[:, None]
        ok = (ids >= 0) & (ids < V) & (torch.arange(S)[None] < n)
        want = torch.zeros(B, V + 1, dtype=torch.bool).scatter_(1, torch.where(ok, ids, V), True)[:, :V]
        start = torch.arange(V).expand(B, V) == 999
        seen = _ref.seen_from_bool(start).to(DEV)
        _native.kernels().seen_tokens_add(ids.to(DEV), seen, lens=None if lens is None else n.view(B).int().to(DEV), vocab_size=V)
        assert torch.equal(seen.cpu(), _ref.seen_from_bool(want | start)), lens


def test_min_p_in_candidate_mode():
    lg = (torch.randn(3, 1000, generator=torch.Generator().manual_seed(0)) * 2).bfloat16().float()
    mask = torch.zeros(3, 1000, dtype=torch.uint8, device=DEV)  # rows: tokens 5, 6, 7 of one sequence, noise row 0
    tok = _native.kernels().sample_logits(lg.to(DEV), do_sample=True, min_p=0.2, seed=1, candidates=True, keep_mask=mask,
                                          counter=torch.tensor([5], device=DEV)).cpu()
    want = torch.cat([_ref.sample_tokens(lg[t:t + 1], seed=1, counter=5 + t, min_p=0.2) for t in range(3)])
    assert torch.equal(tok, want) and torch.equal(mask.cpu().bool(), _ref.sample_filter(lg, min_p=0.2)[1])


def _judge(m, prompt, gen, do_sample, eos=(), row=0, kv=None, chunk=None, theta=1.3, min_new=5):
    """tests/test_spec_decode_gpu.py's rules on the processed scores of the eager cached forward over the tokens
    before: greedy, the chosen score within 0.02 + 0.01 |best| of the best; sampled (noise of batch row ``row``),
    within that file's decisive margin, 2 * LOGIT_TOL * (1 + max |logit|). Up to the row's EOS."""
    from gke_ray_train_amd.models import generation as G
    cache = G.KVCache(m.config, 1, prompt.shape[1] + NEW, DEV, G._kv_dtype(m, kv))
    lg = G._prefill(m, prompt, cache, None, chunk)
    seen = torch.zeros_like(lg, dtype=torch.bool).scatter_(1, prompt, True)
    for t, tok in enumerate(gen):
        sup = eos if t < min_new else ()
        z, keep, _ = _ref.sample_filter(lg, repetition_penalty=theta, seen=seen, min_p=0.1 * do_sample, suppress=sup)
        score = torch.where(keep, z + do_sample * _ref.sample_noise(3, t, row + 1, lg.shape[1], DEV)[row:], -math.inf)
        tol = 2 * LOGIT_TOL * (1 + float(lg.abs().max())) if do_sample else 0.02 + 0.01 * float(score.max().abs())
        assert tok not in sup and float(score[0, tok]) >= float(score.max()) - tol, (t, tok, int(score.argmax()), gen)
        seen[0, tok] = True
        if tok in eos or t + 1 == len(gen):
            break
        lg = G.forward_cached(m, torch.tensor([[tok]], device=DEV), cache)


@pytest.mark.parametrize("path", [dict(device_loop=True), dict(device_loop=False), dict(use_graph=False)], ids=str)
@pytest.mark.parametrize("variant", [dict(), dict(kv_cache_dtype="fp8"), dict(prefill_chunk_size=3), dict(ragged=True)], ids=str)
@pytest.mark.parametrize("name", ["llama-tiny-gqa", "llama-tiny-d64"])
def test_generate(name, variant, path):
    from gke_ray_train_amd.models import build_llama
    m, variant = build_llama(name, device=DEV, dtype=torch.bfloat16, seed=0).eval(), dict(variant)
    lens = (9, 5) if variant.pop("ragged", False) else (9,)
    prompts = [torch.randint(0, 8, (1, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) for n in lens]
    ids = torch.cat([torch.nn.functional.pad(p, (9 - p.shape[1], 0)) for p in prompts])  # left padding
    am = torch.tensor([[0] * (9 - n) + [1] * n for n in lens], device=DEV)
    jkw = dict(kv=variant.get("kv_cache_dtype"), chunk=variant.get("prefill_chunk_size"))
    for do_sample in (False, True):
        kw = dict(do_sample=do_sample, seed=3, pad_token_id=0, repetition_penalty=1.3, min_p=0.1, **variant, **path)
        eos = (int(m.generate(prompts[0], max_new_tokens=1, **kw)[0, -1]),)  # the unconstrained run's first token
        kw.update(max_new_tokens=NEW, eos_token_id=list(eos), attention_mask=am)
        assert len(lens) > 1 or m.generate(ids, **kw).shape[1] == 10  # without min_new_tokens the run stops at once
        new = m.generate(ids, min_new_tokens=5, **kw)[:, 9:]
        for b, p in enumerate(prompts):  # each row as its single-row run would be judged
            _judge(m, p, new[b].tolist(), do_sample, eos, b, **jkw)
    # a strong penalty changes the greedy continuation, as _ref's penalised argmax says: the argument is not swallowed
    plain = m.generate(prompts[0], max_new_tokens=NEW, **variant, **path)[0, 9:].tolist()
    pen = m.generate(prompts[0], max_new_tokens=NEW, repetition_penalty=5.0, **variant, **path)[0, 9:].tolist()
    _judge(m, prompts[0], pen, False, theta=5.0, min_new=0, **jkw)
    assert pen != plain and len(set(plain)) < len(set(pen)), (plain, pen)
