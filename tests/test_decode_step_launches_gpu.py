"""The ordered list of native bindings one captured decode step calls (``GraphDecoder._step_body``
run eagerly), for the three kinds of step: the graph replays exactly this sequence per token, so a
launch added, dropped or reordered by a change to models/generation.py shows here.

The expected lists are literals. They were recorded with this file's proxy from the code as it was
BEFORE the layer steps were merged into one skeleton (two layers of ``llama-tiny-d64``), not from
the code under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

FUSED_LAYER = ["gemv_fused", "attn_decode_d64", "gemv_fused", "gemv_fused", "gemv_fused"]
GENERIC_LAYER = ["rmsnorm_fwd", "gemv", "rope_append", "attn_decode_d64", "gemv", "rmsnorm_fwd", "gemv", "gemv"]
VERIFY_LAYER = ["rmsnorm_fwd", "gemv", "rope_append", "attn_decode_multi_d64", "gemv", "rmsnorm_fwd", "gemv",
                "swiglu_fwd"]


@pytest.fixture(scope="module")
def model():
    from gke_ray_train_amd.models import build_llama
    return build_llama("llama-tiny-d64", device=DEV, dtype=torch.bfloat16, seed=0).eval()


def _step_calls(dec, monkeypatch):
    """The names called on ``_native.kernels()`` during one eager step (the proxy of
    test_ragged_generate_gpu.py, keeping the order)."""
    from gke_ray_train_amd import _native
    C = _native.kernels()
    calls = []

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(C, name)
            if not callable(fn) or name.isupper():
                return fn

            def call(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return call

    with monkeypatch.context() as mp:
        mp.setattr(_native, "kernels", lambda: Proxy())
        dec._step_body()
    torch.cuda.synchronize()
    return calls


def _ids(model):
    g = torch.Generator(device=DEV).manual_seed(0)
    return torch.randint(0, model.config.vocab_size, (1, 12), device=DEV, generator=g)


def test_fused_norm_step_with_sampler(model, monkeypatch):
    from gke_ray_train_amd.models import generation as G
    n = model.config.num_hidden_layers
    dec = G.GraphDecoder(model, 1, 32, sampler=G.SamplerConfig(max_new_tokens=8))
    assert dec.norm_ws is not None
    dec.first_token(dec.prefill(_ids(model)))
    assert _step_calls(dec, monkeypatch) == ["rmsnorm_fwd"] + FUSED_LAYER * n + ["gemv_fused", "sample_logits"]


def test_generic_step_without_sampler(model, monkeypatch):
    from gke_ray_train_amd.models import generation as G
    n = model.config.num_hidden_layers
    monkeypatch.setattr(G, "_GEMV_NORM", False)  # GRT_GEMV_NORM=0
    dec = G.GraphDecoder(model, 1, 32)
    assert dec.norm_ws is None
    dec.prefill(_ids(model))
    assert _step_calls(dec, monkeypatch) == GENERIC_LAYER * n + ["rmsnorm_fwd", "gemv"]


def test_verify_step_with_sampler(model, monkeypatch):
    from gke_ray_train_amd.models import generation as G
    n = model.config.num_hidden_layers
    dec = G.GraphDecoder(model, 1, 32, sampler=G.SamplerConfig(max_new_tokens=8), spec=G.SpecConfig(2))
    dec.first_token(dec.prefill(_ids(model)))
    assert _step_calls(dec, monkeypatch) == VERIFY_LAYER * n + ["rmsnorm_fwd", "gemv", "sample_logits", "spec_advance"]
