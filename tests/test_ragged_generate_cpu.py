"""``generate(..., attention_mask=...)`` on the CPU (fp32): a padded batch of prompts of unequal
length gives every row the tokens and logits that row gives alone, wherever the padding sits and
whatever the pad columns hold; plus the mask's validation, the batch call of ``ByteTokenizer`` and
``run_inference_comparison(batch_size=k)``.

Token equality is exact: the single-row greedy runs of llama-tiny-gqa seed 0 have a top-1 / top-2
margin of at least 6.5e-3 at every step, three orders above fp32 reordering noise.
"""
import json
import os
import sys

import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models import generation as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [3, 7, 5]
S = 7
NEW = 6


def _place(prompts, starts, fill):
    """[B, S] ids with prompt b at columns starts[b] ..., ``fill`` [B, S] everywhere else, and the mask."""
    ids = fill.clone()
    mask = torch.zeros_like(ids)
    for b, (p, a) in enumerate(zip(prompts, starts)):
        ids[b, a:a + len(p)] = p
        mask[b, a:a + len(p)] = 1
    return ids, mask


@pytest.fixture(scope="module")
def setup():
    """Model, the three prompts, random valid ids for the pad columns and each row's run alone."""
    torch.manual_seed(0)
    m = build_llama("llama-tiny-gqa", device="cpu", dtype=torch.float32, seed=0).eval()
    fill = torch.randint(0, m.config.vocab_size, (len(LENS), S))
    prompts = [torch.randint(0, m.config.vocab_size, (n,)) for n in LENS]
    alone = [G.generate(m, p[None], max_new_tokens=NEW)[0, len(p):] for p in prompts]
    return m, prompts, fill, alone


def _left(prompts, fill):
    return _place(prompts, [S - len(p) for p in prompts], fill)


def test_left_padded_batch_equals_each_row_alone(setup):
    m, prompts, fill, alone = setup
    ids, mask = _left(prompts, fill)
    out = G.generate(m, ids, attention_mask=mask, max_new_tokens=NEW)
    assert out.shape == (3, S + NEW) and torch.equal(out[:, :S], ids)
    for b in range(3):
        assert torch.equal(out[b, S:], alone[b]), (b, out[b, S:].tolist(), alone[b].tolist())
    # the ids in the pad columns influence nothing; a bool mask means the same
    ids0, _ = _left(prompts, torch.zeros_like(fill))
    out0 = G.generate(m, ids0, attention_mask=mask.bool(), max_new_tokens=NEW)
    assert torch.equal(out0[:, S:], out[:, S:])


def test_padding_placement_does_not_matter(setup):
    m, prompts, fill, alone = setup
    for starts in ([0, 0, 0], [2, 0, 1]):  # right-padded; padding on both sides
        ids, mask = _place(prompts, starts, fill)
        out = G.generate(m, ids, attention_mask=mask.to(torch.int32), max_new_tokens=NEW)
        assert torch.equal(out[:, :S], ids)
        assert torch.equal(out[:, S:], torch.stack(alone)), starts


def test_teacher_forced_logits_match_single_row(setup):
    """Ragged ``forward_cached`` prefill + 4 one-token steps vs each row alone, at the tolerance
    test_generation_cpu.py uses for cached vs full forward."""
    m, prompts, fill, _ = setup
    steps = 4
    ref, toks = [], []
    for p in prompts:
        cache = G.KVCache(m.config, 1, S + steps, torch.device("cpu"), torch.float32)
        lg = [G.forward_cached(m, p[None], cache)]
        for _ in range(steps):
            lg.append(G.forward_cached(m, lg[-1].argmax(-1)[:, None], cache))
        ref.append(torch.cat(lg))            # [steps + 1, V]
        toks.append(ref[-1].argmax(-1))
    ref, toks = torch.stack(ref, 1), torch.stack(toks, 1)  # [steps + 1, B, V], [steps + 1, B]
    ids, mask = _left(prompts, fill)
    cache = G.KVCache(m.config, 3, S + steps, torch.device("cpu"), torch.float32)
    got = [G.forward_cached(m, ids, cache, attention_mask=mask)]
    assert cache.len == S and cache.lens.tolist() == LENS
    for t in range(steps):
        got.append(G.forward_cached(m, toks[t][:, None], cache))
    assert cache.len == S + steps and cache.lens.tolist() == [n + steps for n in LENS]
    torch.testing.assert_close(torch.stack(got), ref, rtol=1e-4, atol=1e-4)


def test_every_token_is_the_no_cache_argmax_of_its_rows_prefix(setup):
    m, prompts, fill, _ = setup
    ids, mask = _left(prompts, fill)
    out = G.generate(m, ids, attention_mask=mask, max_new_tokens=NEW)
    with torch.no_grad():
        for b, p in enumerate(prompts):
            for t in range(NEW):
                prefix = torch.cat([p, out[b, S:S + t]])[None]
                assert int(m(prefix)["logits"][0, -1].argmax()) == int(out[b, S + t]), (b, t)


def test_trivial_masks_take_todays_path(setup, monkeypatch):
    m, _, fill, _ = setup
    seen = []
    real = G.forward_cached

    def spy(model, ids, cache, attention_mask=None):
        seen.append(attention_mask)
        return real(model, ids, cache, attention_mask)

    monkeypatch.setattr(G, "forward_cached", spy)
    a = G.generate(m, fill, max_new_tokens=NEW)
    b = G.generate(m, fill, attention_mask=torch.ones_like(fill), max_new_tokens=NEW)
    c = G.generate(m, fill, attention_mask=torch.ones(fill.shape, dtype=torch.bool), max_new_tokens=NEW)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert seen and all(x is None for x in seen)


def test_invalid_masks_raise(setup):
    m, prompts, fill, _ = setup
    hole = torch.ones_like(fill)
    hole[1, 3] = 0
    with pytest.raises(ValueError, match="row 1"):
        G.generate(m, fill, attention_mask=hole, max_new_tokens=2)
    empty = torch.ones_like(fill)
    empty[2] = 0
    with pytest.raises(ValueError, match="row 2"):
        G.generate(m, fill, attention_mask=empty, max_new_tokens=2)
    with pytest.raises(ValueError, match="shape"):
        G.generate(m, fill, attention_mask=torch.ones(3, S - 1, dtype=torch.long), max_new_tokens=2)
    ids, mask = _left(prompts, fill)
    cache = G.KVCache(m.config, 3, 2 * S + 2, torch.device("cpu"), torch.float32)
    G.forward_cached(m, ids, cache)
    with pytest.raises(ValueError, match="empty cache"):
        G.forward_cached(m, ids, cache, attention_mask=mask)
    ragged = G.KVCache(m.config, 3, 2 * S + 2, torch.device("cpu"), torch.float32)
    G.forward_cached(m, ids, ragged, attention_mask=mask)
    with pytest.raises(ValueError, match="one token"):
        G.forward_cached(m, ids[:, :2], ragged)


def test_eos_in_one_row_first(setup):
    """EOS ids taken from the single-row outputs so that the rows finish at different steps, the
    last of them before the token budget: a finished row continues with ``pad_token_id``, the
    others run on, and the output ends right after the last row's EOS."""
    m, prompts, fill, alone = setup
    alone = [a.tolist() for a in alone]
    pad = next(i for i in range(m.config.vocab_size) if all(i not in a for a in alone))

    def finish(eos):
        return [next((t for t, x in enumerate(a) if x in eos), None) for a in alone]

    pick = None
    for t0 in range(NEW - 1):
        for t1 in range(NEW - 1):
            for t2 in range(NEW - 1):
                eos = {alone[0][t0], alone[1][t1], alone[2][t2]}
                f = finish(eos)
                if len(set(f)) > 1 and pick is None:
                    pick = (sorted(eos), f)
    assert pick is not None, alone
    eos, f = pick
    n = max(f) + 1
    assert n < NEW
    want = torch.tensor([a[:fb + 1] + [pad] * (n - fb - 1) for a, fb in zip(alone, f)])
    ids, mask = _left(prompts, fill)
    out = G.generate(m, ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad)
    assert out.shape == (3, S + n), (out.shape, f)
    assert torch.equal(out[:, :S], ids) and torch.equal(out[:, S:], want), (out[:, S:].tolist(), want.tolist())


def test_tokenizer_batch_call():
    from gke_ray_train_amd.data.tokenizer import ByteTokenizer
    tok = ByteTokenizer(512)
    tok.pad_token = tok.eos_token
    texts = ["select 1;", "a", "<|eot_id|>rank the rows"]
    enc = [tok.encode(t) for t in texts]
    n = max(len(e) for e in enc)
    for side in ("left", "right"):
        tok.padding_side = side
        for padding in (True, "longest"):
            r = tok(texts, padding=padding, return_tensors="pt")
            ids, mask = r["input_ids"], r["attention_mask"]
            assert ids.shape == mask.shape == (3, n) and ids.dtype == torch.long
            assert mask.sum(1).tolist() == [len(e) for e in enc]
            for b, e in enumerate(enc):
                k = n - len(e)
                real = ids[b, k:] if side == "left" else ids[b, :len(e)]
                pads = ids[b, :k] if side == "left" else ids[b, len(e):]
                ones = mask[b, k:] if side == "left" else mask[b, :len(e)]
                assert real.tolist() == e and bool(ones.all()) and bool((pads == tok.pad_token_id).all())
    tok.pad_token = "<|pad|>"
    r = tok(texts, padding=True)
    assert r["input_ids"][1][-1] == tok.special_ids["<|pad|>"] and r["attention_mask"][1] == [1] + [0] * (n - 1)
    assert tok(texts)["input_ids"] == enc  # no padding asked for: lists of unequal length
    with pytest.raises(ValueError):
        tok(texts, return_tensors="pt")
    # the single-string call is what it was
    one = tok("select 1;", return_tensors="pt")
    assert one["input_ids"].tolist() == [enc[0]] and one["attention_mask"].tolist() == [[1] * len(enc[0])]
    assert tok("select 1;") == {"input_ids": enc[0], "attention_mask": [1] * len(enc[0])}
    assert tok("select 1;", truncation=True, max_length=4)["input_ids"] == enc[0][:4]


def test_inference_comparison_batch_size_2(tmp_path, monkeypatch):
    """Three prompts of unequal length: ``batch_size=2`` makes one ``generate`` call per model and
    chunk (2 + 1 samples), left-padded with a mask whose row sums are the prompt lengths, and writes
    the same ids and prompts in the same order as ``batch_size=1``. (bf16 models on the CPU: the
    response strings are not compared.)"""
    sys.path.insert(0, os.path.join(ROOT, "jobs"))
    import fine_tune_llama_ray as job
    from gke_ray_train_amd.data.tokenizer import ByteTokenizer
    from gke_ray_train_amd.models.llama import LlamaForCausalLM
    from gke_ray_train_amd.trainer.sft_data import format_chat_sample, synthetic_text_to_sql
    m = build_llama("llama-tiny-gqa", device="cpu", dtype=torch.float32, seed=3)
    tok = ByteTokenizer(m.config.vocab_size)
    tok.pad_token = tok.eos_token
    saved = str(tmp_path / "tuned")
    m.save_pretrained(saved)
    tok.save_pretrained(saved)
    rows = [r for r in synthetic_text_to_sql(64, seed=42, split="test") if r["sql_complexity"] == "window functions"][:3]
    lens = [len(tok.encode(format_chat_sample(r, tok, with_answer=False)["text"])) for r in rows]
    assert len(rows) == 3 and lens[0] != lens[1]
    calls = []
    real = LlamaForCausalLM.generate

    def spy(self, input_ids, **kw):
        calls.append((tuple(input_ids.shape), kw.get("attention_mask")))
        return real(self, input_ids, **kw)

    monkeypatch.setattr(LlamaForCausalLM, "generate", spy)
    res = {}
    for bs in (1, 2):
        calls.clear()
        path = job.run_inference_comparison("llama-tiny-gqa", saved, rows, 4096, str(tmp_path / f"bs{bs}"), "cpu",
                                            max_new_generation_tokens=3, tokenizer=tok, batch_size=bs)
        res[bs] = json.load(open(path))
        if bs == 1:  # today's calls: one per sample and model, no mask
            assert [c[0] for c in calls] == [(1, n) for n in lens for _ in range(2)]
            assert all(c[1] is None for c in calls)
        else:  # chunks of 2 + 1 samples, two models each
            assert [c[0] for c in calls] == [(2, max(lens[:2]))] * 2 + [(1, lens[2])] * 2
            for shape, mask in calls[:2]:
                assert mask.sum(1).tolist() == lens[:2]
                short = min(range(2), key=lambda b: lens[b])
                assert mask[short, :shape[1] - lens[short]].sum() == 0  # left-padded
            assert all(c[1] is None for c in calls[2:])
    assert [list(r) for r in res[1]] == [list(r) for r in res[2]]
    for a, b in zip(res[1], res[2]):
        for k in a:
            if not k.endswith("_sql_response"):
                assert a[k] == b[k], k
    assert [r["id"] for r in res[2]] == [r["id"] for r in rows]
