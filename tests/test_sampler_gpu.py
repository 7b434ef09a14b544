"""The device token sampler (csrc/kernels/sample.hip, binding ``sample_logits``) against its host
implementation in float64 (``ops/_ref.py``: ``sample_filter``, ``sample_noise``, ``sample_tokens``).

Comparison rules (set by reasoning, not by what the kernel gives):

* greedy: exact equality with CPU ``torch.argmax`` (first maximum), constructed ties included;
* kept set: with top_p < 1 a token whose reference coordinate ``frac = M_>(i) / Z`` lies within 1e-5
  of top_p (and is not the maximum, which is always kept) may go either way, every other token must
  match. 1e-5 is >= 30x the kernel's error budget (a 1-ulp fp32 exp plus 2^-40 fixed-point truncation
  over 2^17 addends, about 3e-7) and far below one token's probability at these boundaries. On the
  random inputs the test first asserts that the reference has NO token in that band, so the band
  hides nothing there. (V = 1000 with B = 33 is left out of the random grid for that reason: with
  either generator seed one row has a token within 1e-5 of top_p = 0.9.)
* draw: the token equals ``_ref.sample_tokens`` for the same (seed, counter, row), leaving out the
  draws whose two best reference scores differ by less than 1e-4 (fp32 against float64 logs and
  add), which must be at most 1 % of the draws."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIGMA = {1: 2, 7: 2, 512: 2, 1000: 3, 32000: 4, 128256: 4}
# (B, generator seed) per V
SHAPES = {V: ((1, 0), (3, 1), (33, 0)) for V in SIGMA}
SHAPES[1000] = ((1, 0), (3, 1))
DTYPES = [torch.float32, torch.bfloat16]
BIG = 1e30  # fills whatever lies outside the rows: a read past a row would win every argmax


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _ref():
    from gke_ray_train_amd.ops import _ref
    return _ref


def _values(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * SIGMA[V]).bfloat16().float().to(DEV)


def _layout(vals, dtype, kind):
    """The same values as a [B, V] view: ``contig``; ``padded`` (row stride V + 3); ``aligned`` (16-byte
    aligned rows: stride rounded up to 16 bytes); ``offset`` (rows 1 .. B of a [B + 1, V] buffer)."""
    B, V = vals.shape
    if kind == "contig":
        return vals.to(dtype)
    if kind == "offset":
        buf = torch.full((B + 1, V), BIG, device=DEV, dtype=dtype)
        buf[1:] = vals
        return buf[1:]
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    ld = V + 3 if kind == "padded" else (V + per16 - 1) // per16 * per16 + per16
    buf = torch.full((B, ld), BIG, device=DEV, dtype=dtype)
    buf[:, :V] = vals
    view = buf[:, :V]
    if kind == "aligned":
        assert view.data_ptr() % 16 == 0 and (view.stride(0) * view.element_size()) % 16 == 0
    return view


LAYOUTS = ("contig", "padded", "aligned", "offset")


# ------------------------------------------------------------------ greedy
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", sorted(SIGMA))
def test_greedy_is_first_argmax(V, dtype):
    for B, seed in SHAPES[V]:
        vals = _values(B, V, seed)
        top = vals.max(-1, keepdim=True).values
        g = torch.Generator().manual_seed(seed + 10)
        # ties at the maximum: copies of it at random places in every second row
        ties = (torch.rand(B, V, generator=g) < min(0.5, 4.0 / V)).to(DEV) & (torch.arange(B, device=DEV) % 2 == 0)[:, None]
        vals = torch.where(ties, top.expand(B, V), vals)
        want = vals.cpu().argmax(-1)
        idx = torch.arange(V, device=DEV).expand(B, V)
        first = torch.where(vals == top, idx, torch.full_like(idx, V)).min(-1).values
        assert torch.equal(want, first.cpu())  # CPU argmax is the first maximum
        for kind in LAYOUTS:
            got = _C().sample_logits(_layout(vals, dtype, kind))
            assert got.dtype == torch.int64 and got.shape == (B,)
            assert torch.equal(got.cpu(), want), (V, B, kind)


# ------------------------------------------------------------------ kept set
def _check_keep(lg, dtype, kind, T, k, p, assert_empty_band):
    B, V = lg.shape
    z, keep, frac = _ref().sample_filter(lg, T, k, p)
    band = ((frac - p).abs() <= 1e-5) & (frac > 0) if p < 1.0 else torch.zeros_like(keep)
    if assert_empty_band:
        assert int(band.sum()) == 0, f"reference has {int(band.sum())} tokens within 1e-5 of top_p: pick other inputs"
    mask = torch.full((B, V), 7, dtype=torch.uint8, device=DEV)
    tok = _C().sample_logits(_layout(lg, dtype, kind), do_sample=True, temperature=T, top_k=k, top_p=p, seed=1,
                             keep_mask=mask)
    assert int(mask.max()) <= 1
    bad = (mask.bool() != keep) & ~band
    assert not bool(bad.any()), (f"V={V} B={B} {kind} T={T} top_k={k} top_p={p}: {int(bad.sum())} tokens differ, "
                                 f"kernel keeps {mask.sum(-1).tolist()}, reference {keep.sum(-1).tolist()}")
    # the drawn token is a kept one (index 0 when nothing is kept)
    picked = mask.gather(-1, tok[:, None]).squeeze(-1).bool()
    assert bool((picked | ((mask.sum(-1) == 0) & (tok == 0))).all())


def _grid(V):
    return [(T, k, p) for T in (0.7, 1.0) for k in (0, 1, 2, 50, V, V + 1) for p in (1e-6, 0.5, 0.9, 1.0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", sorted(SIGMA))
def test_kept_set_matches_reference(V, dtype):
    n = 0
    for B, seed in SHAPES[V]:
        lg = _values(B, V, seed)
        for T, k, p in _grid(V):
            _check_keep(lg, dtype, LAYOUTS[n % len(LAYOUTS)], T, k, p, assert_empty_band=True)
            n += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [7, 512, 1000])
def test_kept_set_on_ties_and_infinities(V, dtype):
    g = torch.Generator().manual_seed(5)
    few = torch.randint(-3, 4, (V,), generator=g).float() * 0.5     # 7 distinct values: ties straddle every k
    holes = torch.randn(V, generator=g) * 2
    holes[torch.rand(V, generator=g) < 0.3] = -math.inf
    holes[0] = 1.0
    zeros = torch.zeros(V)
    zeros[::2] = -0.0                                                 # +0 and -0 are one tie group
    pair = torch.randn(V, generator=g) * 2
    pair[V // 2:] = pair[:V - V // 2].clone()                               # every value twice (V odd: one thrice)
    rows = [few, holes, torch.full((V,), 1.25), torch.full((V,), -math.inf), zeros, pair.bfloat16().float()]
    lg = torch.stack(rows).bfloat16().float().to(DEV)  # both dtypes hold these values exactly
    for n, (T, k, p) in enumerate(_grid(V)):
        _check_keep(lg, dtype, LAYOUTS[n % len(LAYOUTS)], T, k, p, assert_empty_band=False)
    # -inf is never kept; the all -inf row keeps nothing and returns index 0
    mask = torch.zeros(len(rows), V, dtype=torch.uint8, device=DEV)
    tok = _C().sample_logits(lg.to(dtype), do_sample=True, top_k=V, keep_mask=mask)
    assert not bool(mask.bool()[lg == -math.inf].any()) and int(mask[3].sum()) == 0 and int(tok[3]) == 0
    assert int(mask[2].sum()) == V and int(mask[4].sum()) == V


def test_nan_rows_return_a_valid_index():
    lg = torch.randn(4, 1000, device=DEV)
    lg[0] = math.nan
    lg[1, ::3] = math.nan
    lg[2, 5] = math.inf
    for kw in (dict(), dict(do_sample=True), dict(do_sample=True, top_k=5, top_p=0.5)):
        tok = _C().sample_logits(lg, **kw)
        assert bool(((tok >= 0) & (tok < 1000)).all()), kw
        assert int(tok[0]) == 0 and int(tok[2]) == 5 and not bool(torch.isnan(lg[1, tok[1]])), kw


# ------------------------------------------------------------------ draw
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [7, 512, 1000, 128256])
def test_draw_matches_reference(V, dtype):
    R = _ref()
    B = 33
    lg = _values(B, V, 1)
    counter = torch.zeros(1, dtype=torch.long, device=DEV)
    draws = skipped = 0
    for cfg in (dict(temperature=1.0), dict(temperature=0.7, top_k=50, top_p=0.9), dict(temperature=1.3, top_p=0.5)):
        for seed, c in ((0, 0), (0, 1), (3, 0), (2 ** 62 + 5, 7), (-9, 2 ** 40)):
            counter.fill_(c)
            got = _C().sample_logits(_layout(lg, dtype, "padded"), do_sample=True, seed=seed, counter=counter, **cfg)
            want = R.sample_tokens(lg, seed=seed, counter=c, **cfg)
            z, keep, _ = R.sample_filter(lg, cfg["temperature"], cfg.get("top_k", 0), cfg.get("top_p", 1.0))
            score = torch.where(keep, z + R.sample_noise(seed, c, B, V, DEV), torch.full_like(z, -math.inf))
            if V > 1:
                top2 = score.topk(2, -1).values
                clear = (top2[:, 0] - top2[:, 1]) >= 1e-4
            else:
                clear = torch.ones(B, dtype=torch.bool, device=DEV)
            draws += B
            skipped += int((~clear).sum())
            assert torch.equal(got[clear], want[clear]), (V, cfg, seed, c, got.tolist(), want.tolist())
    print(f"V={V}: {skipped} of {draws} draws left out as near-ties")
    assert skipped <= 0.01 * draws


def test_counter_changes_the_draw_and_launches_are_bitwise_stable():
    V, B = 32000, 3
    lg = _values(B, V, 0).bfloat16()
    counter = torch.zeros(1, dtype=torch.long, device=DEV)
    kw = dict(do_sample=True, temperature=2.0, top_k=0, top_p=0.9, seed=4, counter=counter)
    runs = []
    for c in (0, 0, 1, 2, 3):
        counter.fill_(c)
        mask = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
        runs.append((_C().sample_logits(lg, keep_mask=mask, **kw).clone(), mask))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for tok, mask in runs[2:]:
        assert torch.equal(mask, runs[0][1])  # the kept set does not depend on the counter
    assert int(runs[0][1].sum(-1).min()) >= 100  # every row draws among at least a hundred kept tokens
    toks = [tuple(r[0].tolist()) for r in runs[1:]]  # counters 0, 1, 2, 3
    assert len(set(toks)) == 4 and all(len({t[b] for t in toks}) >= 2 for b in range(B)), toks
    # no counter tensor: counter 0
    assert torch.equal(_C().sample_logits(lg, do_sample=True, temperature=2.0, top_p=0.9, seed=4), runs[0][0])


# ------------------------------------------------------------------ fused epilogue
def test_fused_epilogue_bookkeeping():
    B, V, W = 5, 512, 6
    eos = [3, 11, 12, 13, 14, 15, 16, 500]  # 8 ids
    win = [7, 500, 3, 9, 11]                 # the greedy winners by construction
    lg = torch.zeros(B, V, device=DEV)
    for b, w in enumerate(win):
        lg[b, w] = 5.0
    finished = torch.tensor([False, False, True, True, False], device=DEV)
    finish_step = torch.tensor([-1, -1, 0, 1, -1], device=DEV)
    step = torch.tensor([4], device=DEV)
    out = torch.full((B, W + 2), -7, dtype=torch.long, device=DEV)[:, :W]  # a strided view
    nxt = torch.full((B, 1), -7, dtype=torch.long, device=DEV)
    eos_t = torch.tensor(eos, device=DEV)
    tok = _C().sample_logits(lg, finished=finished, finish_step=finish_step, step=step, next_ids=nxt.view(B), out=out,
                             eos_ids=eos_t, pad_id=0, max_steps=W)
    assert tok.data_ptr() == nxt.data_ptr()
    # rows 2 and 3 were finished: pad, state untouched; rows 1 and 4 hit an EOS id now, at step 4
    assert nxt.view(B).tolist() == [7, 500, 0, 0, 11]
    assert out[:, 4].tolist() == [7, 500, 0, 0, 11]
    assert bool((out[:, [0, 1, 2, 3, 5]] == -7).all())
    assert finished.tolist() == [False, True, True, True, True]
    assert finish_step.tolist() == [-1, 4, 0, 1, 4]
    # without a pad id a finished row keeps emitting its winner; a step past out's width writes no column
    step.fill_(W)
    before = out.clone()
    tok = _C().sample_logits(lg, finished=finished, finish_step=finish_step, step=step, out=out, eos_ids=eos_t,
                             max_steps=W)
    assert tok.tolist() == win and torch.equal(out, before) and finish_step.tolist() == [-1, 4, 0, 1, 4]
    # sampling takes the same epilogue
    step.fill_(0)
    finished.zero_()
    tok = _C().sample_logits(lg * 40, do_sample=True, top_k=1, seed=9, finished=finished, finish_step=finish_step,
                             step=step, out=out, eos_ids=eos_t, pad_id=0, max_steps=W)
    assert tok.tolist() == win and out[:, 0].tolist() == win and finished.tolist() == [False, True, True, False, True]


# ------------------------------------------------------------------ refusals
def test_refusals():
    C = _C()
    lg = torch.randn(2, 64, device=DEV)
    state = dict(finished=torch.zeros(2, dtype=torch.bool, device=DEV),
                 finish_step=torch.zeros(2, dtype=torch.long, device=DEV),
                 step=torch.zeros(1, dtype=torch.long, device=DEV),
                 out=torch.zeros(2, 4, dtype=torch.long, device=DEV))
    C.sample_logits(lg, **state, max_steps=4)  # the well-formed call
    with pytest.raises(RuntimeError, match="bf16/fp32"):
        C.sample_logits(lg.half())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.sample_logits(lg.cpu())
    for t in (0.0, -1.0, math.nan):
        with pytest.raises(RuntimeError, match="temperature"):
            C.sample_logits(lg, do_sample=True, temperature=t)
    for p in (0.0, 1.5, -0.1):
        with pytest.raises(RuntimeError, match="top_p"):
            C.sample_logits(lg, do_sample=True, top_p=p)
    with pytest.raises(RuntimeError, match="top_k"):
        C.sample_logits(lg, do_sample=True, top_k=-1)
    with pytest.raises(RuntimeError, match="at most 8 EOS"):
        C.sample_logits(lg, **state, eos_ids=torch.arange(9, device=DEV), max_steps=4)
    with pytest.raises(RuntimeError, match="too narrow"):
        C.sample_logits(lg, **state, max_steps=5)
    with pytest.raises(RuntimeError, match="last dimension contiguous"):
        C.sample_logits(torch.randn(2, 128, device=DEV)[:, ::2])
    with pytest.raises(RuntimeError, match="row stride"):
        C.sample_logits(lg[:1].expand(2, 64))
    with pytest.raises(RuntimeError, match="come together"):
        C.sample_logits(lg, finished=state["finished"])
    with pytest.raises(RuntimeError, match="int64"):
        C.sample_logits(lg, **{**state, "step": torch.zeros(1, dtype=torch.int32, device=DEV)}, max_steps=4)
    with pytest.raises(RuntimeError, match="keep_mask"):
        C.sample_logits(lg, do_sample=True, keep_mask=torch.zeros(2, 63, dtype=torch.uint8, device=DEV))
