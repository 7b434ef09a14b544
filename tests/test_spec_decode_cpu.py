"""Prompt-lookup speculative decoding on the host: the draft and accept rules of ``ops/_ref.py``
(the oracles of csrc/kernels/spec.hip) on hand-worked cases, and ``generate(...,
prompt_lookup_num_tokens=K)`` on the eager CPU path against the plain run of the same model."""
import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models import generation as G
from gke_ray_train_amd.ops import _ref


# ------------------------------------------------------------------ 1. the draft
def test_draft_longer_ngram_wins_over_a_later_short_match():
    #       0  1  2  3  4  5  6  7
    hist = [5, 6, 7, 9, 6, 8, 5, 6]
    # n = 2: the tail (5, 6) occurs at 0, continuation 7 9 6; n = 1 alone would take the 6 at 4 -> 8 5 6
    assert _ref.prompt_lookup_draft(hist, 8, 3, 2) == [7, 9, 6]
    assert _ref.prompt_lookup_draft(hist, 8, 3, 1) == [8, 5, 6]


def test_draft_latest_match_wins():
    hist = [1, 2, 3, 1, 2, 4, 1, 2]
    assert _ref.prompt_lookup_draft(hist, 8, 2, 2) == [4, 1]
    assert _ref.prompt_lookup_draft(hist, 8, 1, 2) == [4]


def test_draft_continuation_cut_at_the_history_end_pads():
    hist = [1, 2, 3, 1, 2]
    assert _ref.prompt_lookup_draft(hist, 5, 3, 2) == [3, 1, 2]
    hist = [7, 7]              # n = 1: the 7 at 0 continues with one token only
    assert _ref.prompt_lookup_draft(hist, 2, 3, 2) == [7, -1, -1]
    hist = [4, 9, 9, 9]        # n = 2: (9, 9) at 1 overlaps the tail, continuation = the last 9
    assert _ref.prompt_lookup_draft(hist, 4, 3, 2) == [9, -1, -1]
    assert _ref.prompt_lookup_draft(hist + [0, 0], 4, 3, 2) == [9, -1, -1]  # n_hist bounds the read


def test_draft_one_token_history_and_no_match():
    assert _ref.prompt_lookup_draft([3], 1, 3, 2) == [-1, -1, -1]
    assert _ref.prompt_lookup_draft([1, 2, 3, 4], 4, 2, 3) == [-1, -1]
    assert _ref.prompt_lookup_draft(torch.tensor([1, 2, 1]), 3, 2, 4) == [2, 1]


# ------------------------------------------------------------------ 2. the accept step
def test_accept_all():
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 2, 100) == ([4, 5, 6, 7], False, -1)


def test_accept_first_draft_rejected():
    assert _ref.spec_accept([4, 5, 6], [9, 5, 6, 7], 2, 100) == ([9], False, -1)
    assert _ref.spec_accept([4, 5, 6], [4, 8, 6, 7], 2, 100) == ([4, 8], False, -1)  # later agreement is void


def test_accept_stops_at_an_open_slot():
    assert _ref.spec_accept([4, -1, -1], [4, 5, 6, 7], 0, 100) == ([4, 5], False, -1)
    assert _ref.spec_accept([-1, -1, -1], [4, 5, 6, 7], 0, 100) == ([4], False, -1)


def test_accept_eos_in_the_middle_of_an_accepted_run():
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 10, 100, eos_ids=(5,)) == ([4, 5], True, 11)
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 10, 100, eos_ids=(4, 7)) == ([4], True, 10)


def test_accept_cut_at_max_new_tokens():
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 6, 8) == ([4, 5], False, -1)
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 7, 8, eos_ids=(5,)) == ([4], False, -1)


def test_accept_finished_or_full_row_is_inert():
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 3, 100, finished=True) == ([], True, -1)
    assert _ref.spec_accept([4, 5, 6], [4, 5, 6, 7], 8, 8) == ([], False, -1)


# ------------------------------------------------------------------ 3. generate(), eager fp32 on the CPU
S, NEW = 10, 14
MIN_MARGIN = 1e-3  # fp32: a 1-row and a 4-row forward differ by ~1e-6 in the logits


def _plain_run(seed, ids=None):
    """Greedy tokens of the plain eager run and the smallest top-1 / top-2 margin of its steps."""
    m = build_llama("llama-tiny", device="cpu", dtype=torch.float32, seed=seed).eval()
    if ids is None:
        ids = torch.randint(0, m.config.vocab_size, (1, S), generator=torch.Generator().manual_seed(seed))
    cache = G.KVCache(m.config, 1, ids.shape[1] + NEW, "cpu", torch.float32)
    logits = G.forward_cached(m, ids, cache)
    toks, margin = [], float("inf")
    for _ in range(NEW):
        top = logits[0].topk(2).values
        margin = min(margin, float(top[0] - top[1]))
        toks.append(int(logits.argmax(-1)))
        if len(toks) < NEW:
            logits = G.forward_cached(m, torch.tensor([[toks[-1]]]), cache)
    return m, ids, toks, margin


@pytest.fixture(scope="module")
def plain():
    """The model seed is chosen from the plain run alone: the first of seeds 0-9 whose every step
    has a decisive top-1 / top-2 margin, so that no rounding difference can change a token."""
    for seed in range(10):
        m, ids, toks, margin = _plain_run(seed)
        if margin > MIN_MARGIN:
            want = G.generate(m, ids, max_new_tokens=NEW, use_graph=False)
            assert want[0, S:].tolist() == toks
            return m, ids, toks
    pytest.fail("no seed in 0-9 gives a plain run whose every step is decisive")


def _count_forwards(monkeypatch):
    calls = {"n": 0}
    real = G.forward_cached

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(G, "forward_cached", counted)
    return calls


def test_generate_with_a_perfect_plan_takes_fewer_forwards(plain, monkeypatch):
    m, ids, toks = plain
    calls = _count_forwards(monkeypatch)
    out = G.generate(m, ids, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=3,
                     _spec_plan=torch.tensor(toks))
    assert out[0, :S].tolist() == ids[0].tolist() and out[0, S:].tolist() == toks
    assert calls["n"] < NEW, calls
    assert calls["n"] == 1 + -(-(NEW - 1) // 4)  # the prefill, then 4 tokens per verify step
    assert G.last_spec_stats == {"n_replays": calls["n"] - 1, "n_emitted": NEW}
    # the same through the model's method
    assert torch.equal(m.generate(ids, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=3,
                                  _spec_plan=torch.tensor(toks)), out)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_generate_with_a_corrupted_plan_gives_the_plain_tokens(plain, monkeypatch, K):
    m, ids, toks = plain
    bad = list(toks)
    for n in (3, 8):  # two known token numbers: the drafts for them are wrong, the output is not
        bad[n] = (bad[n] + 1) % m.config.vocab_size
    calls = _count_forwards(monkeypatch)
    out = G.generate(m, ids, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=K,
                     _spec_plan=torch.tensor(bad))
    assert out[0, S:].tolist() == toks
    assert calls["n"] < NEW


def test_generate_with_the_real_lookup_gives_the_plain_tokens():
    """A prompt over 4 ids repeats itself, so the lookup drafts at every step (accepted or not)."""
    for seed in range(10):
        ids = torch.randint(0, 4, (1, 24), generator=torch.Generator().manual_seed(100 + seed))
        m, ids, toks, margin = _plain_run(seed, ids)
        if margin > MIN_MARGIN:
            break
    else:
        pytest.fail("no seed in 0-9 gives a plain run whose every step is decisive")
    assert _ref.prompt_lookup_draft(ids[0], 24, 3, 2) != [-1, -1, -1]
    for K, N in ((3, 2), (2, 1), (1, 4)):
        out = G.generate(m, ids, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=K,
                         max_matching_ngram_size=N)
        assert out[0, 24:].tolist() == toks, (K, N)
    # EOS inside the run and a length that is no multiple of K + 1
    eos = toks[5]
    want = G.generate(m, ids, max_new_tokens=NEW - 1, use_graph=False, eos_token_id=eos)
    got = G.generate(m, ids, max_new_tokens=NEW - 1, use_graph=False, eos_token_id=eos, prompt_lookup_num_tokens=3)
    assert torch.equal(got, want) and got.shape[1] == 24 + toks.index(eos) + 1


def test_generate_sampled_and_padded_row(plain):
    m, ids, toks = plain
    kw = dict(max_new_tokens=NEW, use_graph=False, do_sample=True, seed=5, top_k=1)
    assert G.generate(m, ids, prompt_lookup_num_tokens=3, _spec_plan=torch.tensor(toks), **kw)[0, S:].tolist() == toks
    pad = torch.cat([torch.full((1, 3), 7), ids], 1)
    mask = torch.cat([torch.zeros(1, 3, dtype=torch.long), torch.ones(1, S, dtype=torch.long)], 1)
    out = G.generate(m, pad, attention_mask=mask, max_new_tokens=NEW, use_graph=False, prompt_lookup_num_tokens=3,
                     _spec_plan=torch.tensor(toks))
    assert torch.equal(out[:, :S + 3], pad) and out[0, S + 3:].tolist() == toks


def test_generate_refuses_what_it_cannot_do(plain):
    m, ids, _ = plain
    kw = dict(max_new_tokens=4, use_graph=False)
    with pytest.raises(ValueError, match=r"1\.\.3"):
        G.generate(m, ids, prompt_lookup_num_tokens=4, **kw)
    with pytest.raises(ValueError, match=r"1\.\.3"):
        G.generate(m, ids, prompt_lookup_num_tokens=-1, **kw)
    with pytest.raises(ValueError, match="max_matching_ngram_size must be >= 1"):
        G.generate(m, ids, prompt_lookup_num_tokens=2, max_matching_ngram_size=0, **kw)
    with pytest.raises(ValueError, match="batch of 1"):
        G.generate(m, ids.repeat(2, 1), prompt_lookup_num_tokens=2, **kw)
    with pytest.raises(ValueError, match="generator"):
        G.generate(m, ids, prompt_lookup_num_tokens=2, do_sample=True, generator=torch.Generator(), **kw)
    limit = m.config.max_position_embeddings
    with pytest.raises(ValueError, match=f"max_position_embeddings \\({limit}\\)"):
        G.generate(m, ids, prompt_lookup_num_tokens=2, max_new_tokens=limit - S - 1, use_graph=False)
    # off: None and 0 are the plain run
    a = G.generate(m, ids, prompt_lookup_num_tokens=0, **kw)
    assert torch.equal(a, G.generate(m, ids, prompt_lookup_num_tokens=None, **kw))


def test_forward_cached_all_logits_matches_one_token_steps(plain):
    m, ids, toks = plain
    c1 = G.KVCache(m.config, 1, S + 4, "cpu", torch.float32)
    G.forward_cached(m, ids, c1)
    one = [G.forward_cached(m, torch.tensor([[t]]), c1)[0] for t in toks[:4]]
    c2 = G.KVCache(m.config, 1, S + 4, "cpu", torch.float32)
    G.forward_cached(m, ids, c2)
    many = G.forward_cached(m, torch.tensor([toks[:4]]), c2, all_logits=True)
    assert many.shape == (1, 4, m.config.vocab_size) and c2.len == S + 4
    torch.testing.assert_close(many[0], torch.stack(one), atol=1e-4, rtol=1e-4)
