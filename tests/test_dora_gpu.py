"""The DoRA kernels (csrc/kernels/dora.hip) against float64, then a DoRA Llama against the float64 CPU
model of test_dora_cpu.py and the merged model. Accuracy bound of a case: MARGIN times the error of an
fp32 torch evaluation of the direct formula on the same inputs (profiles/dora.md records both)."""
import os
import sys

import pytest
import torch

from gke_ray_train_amd import _native
from gke_ray_train_amd.models import build_llama
from gke_ray_train_amd.models.generation import generate
from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
from gke_ray_train_amd.peft.lora import _base_weight
from gke_ray_train_amd.peft.quant import NF4Linear, set_dequant_cache

sys.path.insert(0, os.path.dirname(__file__))
import test_dora_cpu as base  # noqa: E402  (reference_model, randomise)

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
MARGIN, S = 4.0, 2.0  # bound over the yardstick's error; the adapters' scaling
_C = _native.kernels


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _norm_case(source, r, layout, K):
    """Kernel arguments and the exact bf16 values of W, A, B, m; ||s B A|| is about 10 % of ||W||."""
    g = _gen(7)
    out, targets = (48, [(0, 48)]) if layout == "full" else (192, [(0, 128), (160, 32)])  # q, (k bare), v
    w = (torch.randn(out, K, device=DEV, generator=g) * 0.05).to(BF)
    wsrc = dict(w=w, q=None, absmax=None)
    if source == "strided":
        buf = torch.zeros(out, K + 24, device=DEV, dtype=BF)
        buf[:, :K] = w
        wsrc["w"] = buf[:, :K]
    elif source.startswith("nf4"):
        lin = torch.nn.Linear(K, out, bias=False, device=DEV, dtype=BF)
        lin.weight.data.copy_(w)
        layer = NF4Linear.from_linear(lin, BitsAndBytesConfig(bnb_4bit_use_double_quant=source == "nf4dq"))
        w = layer._dequant()
        wsrc = dict(w=None, q=layer.qweight, absmax=layer._absmax_f32())
    As = [(torch.randn(r, K, device=DEV, generator=g) * 0.05).to(BF) for _ in targets]
    Bs = [(torch.randn(n, r, device=DEV, generator=g) * (0.1 / S / r ** 0.5)).to(BF) for _, n in targets]
    Ms = [(torch.rand(n, device=DEV, generator=g) + 0.5).to(BF) for _, n in targets]
    return out, targets, w, wsrc, As, Bs, Ms


def _direct_c(dtype, w, targets, As, Bs, Ms):
    c = torch.ones(w.shape[0], device=DEV, dtype=dtype)
    for (off, n), a, b, m in zip(targets, As, Bs, Ms):
        c[off:off + n] = m.to(dtype) / (w[off:off + n].to(dtype) + S * b.to(dtype) @ a.to(dtype)).norm(dim=1)
    return c


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("layout", ["full", "qkv"])
@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("source", ["bf16", "strided", "nf4", "nf4dq"])
def test_norm_kernel(source, r, layout, K):
    out, targets, w, wsrc, As, Bs, Ms = _norm_case(source, r, layout, K)
    res = _C().dora_norm(wsrc["w"], wsrc["q"], wsrc["absmax"], As, Bs, Ms, [o for o, _ in targets], out, S, True)
    c, norm = res  # an empty list: the kernel refused a shape it is built for
    c64 = _direct_c(torch.float64, w, targets, As, Bs, Ms)
    yard = ((_direct_c(torch.float32, w, targets, As, Bs, Ms).double() - c64).abs() / c64).max().item()
    err = ((c.double() - c64).abs() / c64).max().item()
    print(f"dora_norm {source} r={r} {layout} in={K}: kernel {err:.3e} yardstick {yard:.3e}")
    assert err <= MARGIN * yard
    for (off, n), m in zip(targets, Ms):
        assert torch.allclose(norm[off:off + n] * c[off:off + n], m.float(), rtol=1e-5)  # the norm output
    assert layout == "full" or (c[128:160] == 1).all()  # the untargeted k rows


def test_norm_kernel_ignores_stale_lds():
    C, got = _C(), []
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    out, targets, _, wsrc, As, Bs, Ms = _norm_case("nf4", 64, "qkv", 192)
    for pat in (0x7FC07FC0, 0):  # bf16 NaN pairs (an fp32 NaN as well), then zeros
        C.lds_fill(pat, torch.cuda.current_device())
        got.append(C.dora_norm(None, wsrc["q"], wsrc["absmax"], As, Bs, Ms, [o for o, _ in targets], out, S, False)[0])
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], got[1])


@pytest.mark.parametrize("out", [48, 192])
@pytest.mark.parametrize("tokens", [1, 33, 257])
def test_scale_forward_backward(tokens, out):
    g = _gen(11)
    C = _C()
    u = torch.randn(tokens, out, device=DEV, generator=g).to(BF)
    dy = torch.randn(tokens, out, device=DEV, generator=g).to(BF)
    c = torch.rand(out, device=DEV, generator=g) + 0.5
    m = (torch.rand(out - 16, device=DEV, generator=g) + 0.5).to(BF)  # one target: columns 16 .. out
    m[3] = 0
    y = u.clone()
    C.dora_scale(y, c)
    assert torch.equal(y, (u.float() * c).to(BF))
    du, dm = C.dora_scale_bwd(dy, y, c, [m], [16])
    assert torch.equal(du, (dy.float() * c).to(BF))
    assert torch.equal(dm, C.dora_scale_bwd(dy, y, c, [m], [16])[1])  # run-to-run bitwise
    assert (dm[:16] == 0).all() and dm[16 + 3] == 0  # no target / m == 0
    live = m != 0
    dm64 = ((dy.double() * y.double()).sum(0)[16:] / m.double())[live]
    yard32 = ((dy.float() * y.float()).sum(0)[16:] / m.float())[live]
    scale = dm64.abs().max()
    yard = ((yard32.double() - dm64).abs().max() / scale).item()
    err = ((dm[16:][live].double() - dm64).abs().max() / scale).item()
    print(f"dora_scale_bwd tokens={tokens} out={out}: kernel {err:.3e} yardstick {yard:.3e}")
    assert err <= MARGIN * yard


def _dora_llama(nf4):
    m = build_llama("llama-tiny-gqa", device=DEV, dtype=BF, seed=2)
    if nf4:
        quantize_model_(m, BitsAndBytesConfig())
        set_dequant_cache(m, "0")
    pm = get_peft_model(m, LoraConfig(r=16, lora_alpha=16, use_dora=True))
    base.randomise(pm, seed=9)
    return pm


@pytest.mark.parametrize("nf4", [False, True])
def test_training_step_matches_float64_cpu_model(nf4):
    """down_proj (in = 1376) is off the norm kernel's 64-column steps and takes the torch form. Bounds:
    test_lora_small_rank_gpu.py's for the same quantities; the magnitude gradient is held to lora_B's."""
    pm = _dora_llama(nf4)
    ref = base.reference_model(pm, {n: _base_weight(m.base) for n, m in pm.lora_modules.items()})
    ids = torch.randint(0, 512, (2, 256), device=DEV, generator=_gen(4))
    loss, rloss = pm(ids, labels=ids)["loss"], ref(ids.cpu(), labels=ids.cpu())["loss"]
    loss.backward()
    rloss.backward()
    l1, l0 = float(loss.detach()), float(rloss.detach())
    print(f"dora step nf4={nf4}: loss {l1:.6f} vs {l0:.6f}")
    assert abs(l1 - l0) < 1e-3 * max(1.0, abs(l0))
    want, worst = dict(ref.named_parameters()), {}
    for n, p in ((n, p) for n, p in pm.named_parameters() if p.requires_grad):
        g0, kind = want[n].grad, n.split(".lora_")[1].split(".")[0]
        rel = ((p.grad.double().cpu() - g0).norm() / g0.norm().clamp_min(1e-8)).item()
        worst[kind] = max(worst.get(kind, 0.0), rel)
    print(f"dora step nf4={nf4}: worst relative gradient error {worst}")
    assert set(worst) == {"A", "B", "magnitude_vector"} and all(v < 2e-2 for v in worst.values()), worst


def test_generate_matches_merged_model():
    """Greedy generate() of the NF4 DoRA model (graph path, cached c, scale kernel after the product
    from the codes) gives the merged model's tokens. The two models differ by up to 0.02 in a logit; of
    prompt seeds 0-63, 22 has the merged model's largest smallest top-2 gap over the 16 steps (0.375)."""
    pm = _dora_llama(True).eval()
    ids = torch.randint(0, 512, (1, 24), device=DEV, generator=_gen(22))
    got = pm.generate(ids, max_new_tokens=16, do_sample=False)
    assert any(m._dora_c is not None for m in pm.lora_modules.values())
    want = generate(pm.merge_and_unload(), ids, max_new_tokens=16, do_sample=False)
    assert got.shape == (1, 40) and torch.equal(got, want)
