"""DoRA (``LoraConfig(use_dora=True)``) on the CPU: a LoRA Llama against a float64 model whose adapted
projections evaluate the definition directly (materialise W + s B A, detach the row norms)."""
import copy
import functools

import pytest
import torch

from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.peft import LoraConfig, get_peft_model


def direct_forward(mod, w, x):
    """y = m / ||W + s B A|| (.) (x W^T + s x A^T B^T) per target, in x's dtype (float64 here)."""
    y = x @ w.t()
    out = y.clone()
    for name, off, n in mod.targets:
        a, b, m = mod.lora_A[name], mod.lora_B[name], mod.lora_magnitude_vector[name]
        norm = (w[off:off + n] + mod.scaling * b @ a).norm(dim=1).detach()
        out[..., off:off + n] = (m / norm) * (y[..., off:off + n] + mod.scaling * (x @ a.t()) @ b.t())
    return out


def reference_model(pm, weights=None):
    """float64 CPU copy of the DoRA model ``pm``; ``weights`` (module name -> W): a quantised base's W."""
    ref = copy.deepcopy(pm).to("cpu").double()
    for name, mod in ref.lora_modules.items():
        w = (weights[name] if weights else mod.base.weight).detach().to("cpu").double()
        mod.forward = functools.partial(direct_forward, mod, w)
    return ref


def randomise(pm, seed=1):
    """Nonzero B and magnitudes off their initial value, so every term of the formulas counts."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in pm.lora_modules.values():
            for n in mod.lora_B:
                b, m = mod.lora_B[n], mod.lora_magnitude_vector[n]
                b.copy_(torch.randn(b.shape, generator=g) * 0.05)
                m.mul_((1 + 0.2 * torch.randn(m.shape, generator=g)).to(m))


def _model(targets=None, **kw):
    m = build_llama("llama-tiny", device="cpu", dtype=torch.float32, seed=3)
    return get_peft_model(m, LoraConfig(r=8, lora_alpha=16, target_modules=targets, **kw))


@pytest.mark.parametrize("targets", [None, ["q_proj", "v_proj", "down_proj"]])
def test_forward_and_gradients_match_float64(targets):
    pm = _model(targets, use_dora=True)
    for mod in pm.lora_modules.values():  # magnitudes start at the row norms of W
        for name, off, n in mod.targets:
            assert torch.allclose(mod.lora_magnitude_vector[name], mod.base.weight[off:off + n].norm(dim=1), rtol=1e-5)
    randomise(pm)
    ref = reference_model(pm)
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(0))
    out, rout = pm(ids, labels=ids), ref(ids, labels=ids)
    with torch.no_grad():
        assert torch.allclose(pm(ids)["logits"].double(), ref(ids)["logits"], rtol=1e-4, atol=1e-4)
    assert abs(float(out["loss"].detach()) - float(rout["loss"].detach())) < 1e-5
    out["loss"].backward()
    rout["loss"].backward()
    want = dict(ref.named_parameters())
    trained = {n: p for n, p in pm.named_parameters() if p.requires_grad}
    assert any("lora_magnitude_vector" in n for n in trained) and any("lora_A" in n for n in trained)
    for n, p in trained.items():
        assert (p.grad.double() - want[n].grad).norm() <= 1e-4 * want[n].grad.norm() + 1e-9, n


def test_input_gradient_of_a_partly_targeted_module():
    pm = _model(["q_proj", "v_proj"], use_dora=True)  # fused q/k/v, the k rows pass through
    randomise(pm)
    name, mod = next(iter(pm.lora_modules.items()))
    rmod = reference_model(pm).lora_modules[name]
    x = torch.randn(5, mod.in_features, generator=torch.Generator().manual_seed(2), requires_grad=True)
    xr = x.detach().double().requires_grad_(True)
    mod(x).square().sum().backward()
    rmod.forward(xr).square().sum().backward()
    assert torch.allclose(x.grad.double(), xr.grad, rtol=1e-4, atol=1e-5)


def test_save_load_merge_round_trip(tmp_path):
    pm = _model(use_dora=True)
    randomise(pm)
    ids = torch.randint(0, 512, (1, 16), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = pm(ids)["logits"]
    pm.save_pretrained(str(tmp_path))
    assert '"use_dora": true' in (tmp_path / "adapter_config.json").read_text()
    sd = pm.adapter_state_dict()
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_magnitude_vector" in sd
    fresh = _model(use_dora=True)
    fresh.load_adapter(str(tmp_path))
    with torch.no_grad():
        assert torch.allclose(fresh(ids)["logits"], want, atol=1e-6)
        merged = fresh.merge_and_unload()
        assert torch.allclose(merged(ids)["logits"], want, rtol=1e-4, atol=1e-4)


def test_plain_lora_has_no_magnitudes_and_dora_rejects_its_checkpoint():
    plain = _model(use_dora=False)
    sd = plain.adapter_state_dict()
    assert sd and not any("magnitude" in k for k in sd)
    assert not any("magnitude" in n for n, _ in plain.named_parameters())
    with pytest.raises(KeyError, match="lora_magnitude_vector"):
        _model(use_dora=True).load_adapter_state_dict(sd)
