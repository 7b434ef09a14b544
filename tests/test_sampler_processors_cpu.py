"""``_ref``'s logits processors against float64 HF processors; CPU ``generate`` against a full-recompute loop."""
import math

import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.ops import _ref


@pytest.mark.parametrize("theta,min_p,k,p", [(1.3, 0.05, 0, 1.0), (0.7, 0.3, 40, 0.9), (2.0, 1.0, 0, 1.0)])
def test_ref_matches_float64_processors(theta, min_p, k, p):
    B, V, T, sup = 4, 300, 0.7, [3, 250]
    g = torch.Generator().manual_seed(1)
    lg = torch.randn(B, V, generator=g) * 3
    seen = torch.rand(B, V, generator=g) < 0.3
    x = lg.double()
    x[:, sup] = -math.inf
    x = torch.where(seen, torch.where(x < 0, x * theta, x / theta), x) / T       # RepetitionPenalty, Temperature
    if k:
        x = torch.where(x < x.topk(k, -1).values[:, -1:], -math.inf, x)          # TopK
    sp, si = x.sort(-1)                                                           # TopP: ascending, drop cum <= 1 - p
    drop = torch.zeros(B, V, dtype=torch.bool).scatter(1, si, sp.softmax(-1).cumsum(-1) <= 1 - p)
    x = torch.where(drop, -math.inf, x)
    probs = x.softmax(-1)                                                         # MinP
    want = (probs >= min_p * probs.max(-1, keepdim=True).values) & (x > -math.inf)
    for s in (seen, _ref.seen_from_bool(seen)):
        z, keep, _ = _ref.sample_filter(lg, T, k, p, repetition_penalty=theta, seen=s, min_p=min_p, suppress=sup)
        assert torch.equal(keep, want)
        torch.testing.assert_close(z[keep], x[keep], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("do_sample", [False, True])
def test_generate_matches_a_full_recompute_loop(do_sample):
    m = build_llama("llama-tiny", device="cpu", dtype=torch.float32, seed=0).eval()
    ids = torch.randint(0, 6, (1, 7), generator=torch.Generator().manual_seed(0))
    kw = dict(do_sample=do_sample, seed=5, use_graph=False, repetition_penalty=1.3, min_p=0.1)
    eos = [int(m.generate(ids, max_new_tokens=1, **kw)[0, -1])]  # the first token, were it not suppressed
    seq = ids
    for t in range(8):
        seen = torch.zeros(1, m.config.vocab_size, dtype=torch.bool).scatter_(1, seq, True)
        nxt = _ref.sample_tokens(m(seq, return_logits=True)["logits"][:, -1].float(), seed=5, counter=t, do_sample=do_sample,
                                 seen=seen, suppress=eos if t < 4 else (), repetition_penalty=1.3, min_p=0.1 * do_sample)
        seq = torch.cat([seq, nxt[:, None]], 1)
    got = m.generate(ids, max_new_tokens=8, eos_token_id=eos, min_new_tokens=4, **kw)
    n = got.shape[1]  # the run stops right after an EOS, which cannot come before token 4
    assert n > 7 + 4 and eos[0] not in got[0, 7:11].tolist() and torch.equal(got, seq[:, :n])


def test_value_errors():
    m, ids = build_llama("llama-tiny", device="cpu", dtype=torch.float32, seed=0).eval(), torch.zeros(1, 4, dtype=torch.long)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(min_p=1.5), dict(min_p=-0.1),
               dict(min_new_tokens=-1), dict(min_new_tokens=9), dict(repetition_penalty=1.2, prompt_lookup_num_tokens=2),
               dict(min_new_tokens=2, prompt_lookup_num_tokens=2)):
        with pytest.raises(ValueError):
            m.generate(ids, max_new_tokens=8, use_graph=False, **kw)
    m.generate(ids, max_new_tokens=4, use_graph=False, do_sample=True, seed=1, min_p=0.2, prompt_lookup_num_tokens=2)
