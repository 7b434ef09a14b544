"""The host side of the fp8 flash prefill: ``ops.prefill_attention_fp8`` on the CPU is the math
attention over the dequantised rows with the chunk's token rule, and ``prefill_chunk_size`` feeds the
prompt through ``forward_cached`` in chunks (tiny fp32 Llama of test_kv_fp8_cpu.py)."""
import pytest
import torch

from gke_ray_train_amd import ops
from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models import generation as G
from gke_ray_train_amd.ops import _ref


@pytest.mark.parametrize("S,n", [(1, 9), (5, 5), (6, 17)])
def test_cpu_op_is_ref_attention_over_the_dequantised_rows(S, n):
    g = torch.Generator().manual_seed(S + n)
    q = torch.randn(2, S, 4, 64, generator=g)
    (kc, ks), (vc, vs) = (_ref.kv_fp8_quantize(torch.randn(2, n, 2, 64, generator=g)) for _ in range(2))
    kd, vd = _ref.kv_fp8_dequantize(kc, ks), _ref.kv_fp8_dequantize(vc, vs)
    o = ops.prefill_attention_fp8(q, kc, vc, ks, vs)
    assert torch.equal(o, _ref.attention(q, kd, vd, causal=True))
    # the token rule, spelled out: token t alone over its keys [0, n - (S - 1 - t))
    for t in range(S):
        m = n - (S - 1 - t)
        want = _ref.attention(q[:, t:t + 1], kd[:, :m], vd[:, :m], causal=False)
        torch.testing.assert_close(o[:, t:t + 1], want, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("kv", [None, "fp8"])
def test_prefill_chunk_size_feeds_the_prompt_in_chunks(kv):
    m = build_llama("llama-tiny-gqa", device="cpu", dtype=torch.float32, seed=0).eval()
    ids = torch.randint(0, m.config.vocab_size, (2, 11), generator=torch.Generator().manual_seed(3))
    cache = G.KVCache(m.config, 2, 16, "cpu", G._kv_dtype(m, kv))
    for part in (ids[:, :4], ids[:, 4:8], ids[:, 8:]):
        want = G.forward_cached(m, part, cache)
    chunked = G.KVCache(m.config, 2, 16, "cpu", G._kv_dtype(m, kv))
    assert torch.equal(G._prefill(m, ids, chunked, None, 4), want) and chunked.len == 11
    out = G.generate(m, ids, max_new_tokens=3, kv_cache_dtype=kv, prefill_chunk_size=4)
    assert out.shape == (2, 14) and int(out[0, 11]) == int(want[0].argmax())
    assert torch.equal(G.generate(m, ids, max_new_tokens=3, kv_cache_dtype=kv, prefill_chunk_size=None),
                       G.generate(m, ids, max_new_tokens=3, kv_cache_dtype=kv))


@pytest.mark.parametrize("bad", [0, -2, 2.0, "8", True])
def test_prefill_chunk_size_refusals(bad):
    m = build_llama("llama-tiny-gqa", device="cpu", dtype=torch.float32, seed=0).eval()
    ids = torch.tensor([[3, 4, 5, 6, 7]])
    with pytest.raises(ValueError, match="prefill_chunk_size"):
        G.generate(m, ids, max_new_tokens=2, prefill_chunk_size=bad)
    with pytest.raises(ValueError, match="one causal block"):
        G.generate(m, torch.cat([ids, ids]), max_new_tokens=2, prefill_chunk_size=2,
                   attention_mask=torch.tensor([[1] * 5, [0, 0, 1, 1, 1]]))
