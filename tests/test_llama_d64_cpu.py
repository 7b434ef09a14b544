"""head_dim-64 Llama configs: Llama-3.2-1B geometry and the tiny test config (CPU)."""
import pytest
import torch


@pytest.mark.parametrize("name", ["llama3.2-1b", "meta-llama/Llama-3.2-1B"])
def test_llama32_1b_config(name):
    from gke_ray_train_amd.models import get_config
    cfg = get_config(name)
    assert cfg.head_dim == 64
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads) == (2048, 32, 8)
    assert (cfg.vocab_size, cfg.intermediate_size, cfg.num_hidden_layers) == (128256, 8192, 16)
    assert cfg.tie_word_embeddings and cfg.rope_theta == 500000.0 and cfg.max_position_embeddings == 131072
    assert cfg.rope_scaling == dict(type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                    original_max_position_embeddings=8192)
    assert (cfg.bos_token_id, cfg.eos_token_id) == (128000, 128001)
    # tied embeddings counted once
    assert abs(cfg.num_params() - 1.236e9) < 0.01 * 1.236e9


def test_llama_tiny_d64_forward_backward_cpu():
    from gke_ray_train_amd.models import build_llama, get_config
    cfg = get_config("llama-tiny-d64")
    assert cfg.head_dim == 64 and cfg.num_attention_heads == 4 and cfg.num_key_value_heads == 2
    m = build_llama("llama-tiny-d64", device="cpu", dtype=torch.float32, seed=1)
    ids = torch.randint(0, cfg.vocab_size, (2, 32), generator=torch.Generator().manual_seed(0))
    loss = m(ids, labels=ids)["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(g.abs().max() > 0 for g in grads)
