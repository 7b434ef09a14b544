"""The token sampler's host implementation (``ops/_ref.py``: ``sample_noise``, ``sample_filter``,
``sample_tokens``), which is the oracle of csrc/kernels/sample.hip, and ``generate()``'s ``top_k`` /
``seed`` parameters on the CPU path."""
import math

import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models import generation as G
from gke_ray_train_amd.ops import _ref

ROW = torch.tensor([1.5, -0.5, 0.25, 2.0, 0.0, -1.0, 1.0, 0.75])


def test_noise_is_a_pure_function_of_seed_counter_row_index():
    a = _ref.sample_noise(7, 3, 4, 100)
    assert torch.equal(a, _ref.sample_noise(7, 3, 4, 100))
    assert torch.equal(a[:2, :50], _ref.sample_noise(7, 3, 2, 50))  # element (row, i) does not depend on B, V
    assert not torch.equal(a, _ref.sample_noise(7, 4, 4, 100))
    assert not torch.equal(a, _ref.sample_noise(8, 3, 4, 100))
    assert not torch.equal(a[0], a[1])
    # u = (n + 0.5) 2^-23 with n < 2^23: g inside [-log(log(2^24)), -log(-log(1 - 2^-24))]
    assert a.min().item() >= -math.log(24 * math.log(2)) and a.max().item() <= -math.log(-math.log1p(-2.0 ** -24))
    # one scalar recomputed by hand from the recipe in the docstring
    key = _ref._splitmix64_any((_ref._splitmix64_any(7) + 3) & _ref._M64)
    n = _ref._splitmix64_any(key ^ ((2 << 32) | 5)) >> 41
    assert a[2, 5].item() == pytest.approx(-math.log(-math.log((n + 0.5) * 2.0 ** -23)), rel=1e-12)


def test_draws_follow_the_filtered_softmax():
    """20,000 draws (rows 0 .. 19,999 of one launch, seed 1234, counter 0) of an 8-entry row at
    temperature 0.8 with top_k = 5: nothing outside the kept set is drawn and the counts fit the
    renormalised softmax of the kept five. Observed chi-square statistic 4.2226 (4 degrees of
    freedom); the bound is 18.47, the 99.9 % point of that distribution, 4.4x the observed value.
    The test is deterministic given the seed."""
    N = 20000
    tok = _ref.sample_tokens(ROW.expand(N, 8).contiguous(), seed=1234, counter=0, temperature=0.8, top_k=5)
    z, keep, _ = _ref.sample_filter(ROW[None], 0.8, 5, 1.0)
    keep = keep[0]
    assert keep.tolist() == [True, False, True, True, False, False, True, True]
    cnt = torch.bincount(tok, minlength=8).double()
    assert cnt[~keep].sum().item() == 0
    e = torch.where(keep, torch.exp(z[0] - z[0].max()), torch.zeros(8, dtype=torch.float64))
    expect = e / e.sum() * N
    chi2 = (((cnt - expect) ** 2)[keep] / expect[keep]).sum().item()
    print(f"chi-square {chi2:.4f}")
    assert chi2 < 18.47


def test_tie_rules():
    # duplicates straddling the k-th place stay together (top_k = 2 keeps the 3.0 and both 2.0s)
    row = torch.tensor([[2.0, 3.0, 1.0, 2.0, -1.0, 0.0]])
    _, keep, _ = _ref.sample_filter(row, 1.0, 2, 1.0)
    assert keep[0].tolist() == [True, True, False, True, False, False]
    # a tie group is kept or dropped whole by top-p; the maximum always stays
    _, keep, frac = _ref.sample_filter(row, 1.0, 0, 0.6)
    assert keep[0, 0] == keep[0, 3] and keep[0, 1] and frac[0, 0] == frac[0, 3] and frac[0, 1] == 0
    # all equal: everything is kept whatever k and p say
    _, keep, _ = _ref.sample_filter(torch.zeros(1, 9), 0.7, 3, 1e-6)
    assert keep.all()
    # -inf is never kept, and -0.0 ties with +0.0
    row = torch.tensor([[0.0, -0.0, -math.inf, -1.0]])
    _, keep, _ = _ref.sample_filter(row, 1.0, 1, 1.0)
    assert keep[0].tolist() == [True, True, False, False]
    _, keep, _ = _ref.sample_filter(row, 1.0, 4, 1.0)
    assert keep[0].tolist() == [True, True, False, True]
    # greedy and the draw take the lowest index among equal scores; nothing kept -> index 0
    assert _ref.sample_tokens(torch.tensor([[1.0, 5.0, 5.0, 2.0]]), do_sample=False).tolist() == [1]
    assert _ref.sample_tokens(torch.full((2, 5), -math.inf), seed=1).tolist() == [0, 0]
    assert _ref.sample_tokens(torch.full((2, 5), -math.inf), do_sample=False).tolist() == [0, 0]


@pytest.mark.parametrize("kw", [dict(top_k=1), dict(top_p=1e-6)])
def test_top_k_1_and_tiny_top_p_are_argmax(kw):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(16, 1000, generator=g) * 3
    for counter in range(3):
        tok = _ref.sample_tokens(logits, seed=5, counter=counter, temperature=0.7, **kw)
        assert torch.equal(tok, logits.argmax(-1))


def _tiny():
    torch.manual_seed(0)
    m = build_llama("llama-tiny", device="cpu", dtype=torch.float32, seed=0).eval()
    return m, torch.randint(0, m.config.vocab_size, (2, 6))


def test_generate_top_k_1_is_greedy():
    m, ids = _tiny()
    greedy = G.generate(m, ids, max_new_tokens=6)
    assert torch.equal(G.generate(m, ids, max_new_tokens=6, do_sample=True, top_k=1, seed=11), greedy)
    # the torch.multinomial path (a caller's generator) honours top_k too
    g = torch.Generator().manual_seed(3)
    assert torch.equal(G.generate(m, ids, max_new_tokens=6, do_sample=True, top_k=1, generator=g), greedy)


def test_generate_seed_reproduces_and_matters():
    m, ids = _tiny()
    kw = dict(max_new_tokens=12, do_sample=True, temperature=1.5, top_k=50, top_p=0.95)
    a = G.generate(m, ids, seed=3, **kw)
    assert torch.equal(a, G.generate(m, ids, seed=3, **kw))
    assert not torch.equal(a, G.generate(m, ids, seed=4, **kw))
    # seed=None: drawn from torch's default generator, so torch.manual_seed governs the run
    torch.manual_seed(21)
    b = G.generate(m, ids, **kw)
    torch.manual_seed(21)
    assert torch.equal(b, G.generate(m, ids, **kw))
    with pytest.raises(ValueError, match="device_loop"):
        G.generate(m, ids, max_new_tokens=2, device_loop=True)  # no graph path on the CPU
    with pytest.raises(ValueError, match="top_p"):
        G.generate(m, ids, max_new_tokens=2, do_sample=True, top_p=0.0)
