"""The LoRA kernels for ranks 8 / 16 / 32 (csrc/kernels/lora_small.hip) against plain fp32 PyTorch
products of the same bf16 inputs, on the row-strided views the LoRA forward / backward pass; then a
LoRA Llama at r = 8 / 16 on the hot path vs the library fall-backs, and r = 4 (library path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def _C():
    from gke_ray_train_amd import _native
    return _native.kernels()


def _check(got, ref, what, tol=1e-2):
    got, ref = got.float(), ref.float()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    scale = ref.abs().max().clamp_min(1e-6)
    # every element: bf16 output rounding (2^-8 relative) of values up to the tensor's max
    assert (err / scale).max().item() < tol, f"{what}: max err {err.max().item():.4g} vs scale {scale.item():.4g}"


@pytest.mark.parametrize("r", [8, 16, 32])
@pytest.mark.parametrize("M,K", [(96, 256), (200, 1024), (1056, 128)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_g(r, M, K, accumulate):
    torch.manual_seed(0)
    a = torch.randn(M, K + 256, device=DEV, dtype=BF)[:, 128:128 + K]          # column block of dY
    bt = (torch.randn(3 * r, K + 512, device=DEV, dtype=BF) * 0.05)[r:2 * r, 256:256 + K]  # of the B^T buffer
    gbuf = torch.randn(M, 3 * r, device=DEV, dtype=BF)
    c, before = gbuf[:, r:2 * r], gbuf.clone()
    ref = 0.25 * (a.float() @ bt.float().t()) + (before[:, r:2 * r].float() if accumulate else 0)
    assert _C().lora_small_g_group([a], [bt], [c], 0.25, accumulate)
    _check(c, ref, f"g r{r} M{M} K{K} acc{accumulate}")
    assert torch.equal(gbuf[:, :r], before[:, :r]) and torch.equal(gbuf[:, 2 * r:], before[:, 2 * r:])


@pytest.mark.parametrize("r,M", [(8, 200), (16, 1056)])
def test_g_group(r, M):
    torch.manual_seed(3)
    ns = [(0, 512), (512, 128), (640, 256)]  # (offset, width) of the targets in the fused dY
    dy = torch.randn(M, 896, device=DEV, dtype=BF)
    btbuf = torch.randn(3 * r, 896, device=DEV, dtype=BF) * 0.05
    g = torch.randn(M, 3 * r, device=DEV, dtype=BF)
    a = [dy[:, o:o + n] for o, n in ns]
    bt = [btbuf[r * j:r * (j + 1), o:o + n] for j, (o, n) in enumerate(ns)]
    c = [g[:, r * j:r * (j + 1)] for j in range(3)]
    assert _C().lora_small_g_group(a, bt, c, 0.5, False)
    for j in range(3):
        _check(c[j], 0.5 * (a[j].float() @ bt[j].float().t()), f"g_group r{r} M{M} product {j}")


@pytest.mark.parametrize("M,N,R", [(72, 128, 8), (200, 256, 24), (1056, 384, 48), (384, 128, 96), (96, 256, 16)])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_tred(M, N, R, transpose, accumulate):
    torch.manual_seed(1)
    a = torch.randn(M, N + 128, device=DEV, dtype=BF)[:, 128:]
    h = torch.randn(M, R + 64, device=DEV, dtype=BF)[:, :R]
    out = torch.randn((R, N) if transpose else (N, R), device=DEV, dtype=BF)
    ref = a.float().t() @ h.float()
    ref = (ref.t() if transpose else ref) + (out.float() if accumulate else 0)
    assert _C().lora_small_tred(a, h, out, 1.0, accumulate, transpose)
    _check(out, ref, f"tred M{M} N{N} R{R} T{transpose} acc{accumulate}")


def test_tred_group():
    """dB_i of a fused module's targets in one launch, into slot-like views of one flat buffer."""
    torch.manual_seed(4)
    M, r, ns = 200, 16, [(0, 512), (512, 128), (640, 256)]
    dy = torch.randn(M, 896, device=DEV, dtype=BF)
    hc = torch.randn(M, 3 * r, device=DEV, dtype=BF)
    flat = torch.randn(896 * r + 64, device=DEV, dtype=BF)
    outs = [flat[32 + o * r:32 + (o + n) * r].view(n, r) for o, n in ns]
    before, acc = flat.clone(), [False, True, False]
    a = [dy[:, o:o + n] for o, n in ns]
    h = [hc[:, r * j:r * (j + 1)] for j in range(3)]
    assert _C().lora_small_tred_group(a, h, outs, 1.0, acc)
    for j, (o, n) in enumerate(ns):
        old = before[32 + o * r:32 + (o + n) * r].view(n, r).float()
        _check(outs[j], a[j].float().t() @ h[j].float() + (old if acc[j] else 0), f"tred_group product {j}")
    assert torch.equal(flat[:32], before[:32]) and torch.equal(flat[-32:], before[-32:])


@pytest.mark.parametrize("R", [8, 16, 24, 48])
@pytest.mark.parametrize("M,K", [(40, 128), (300, 1024)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_down(R, M, K, p):
    torch.manual_seed(2)
    C = _C()
    buf = torch.randn(M, K + R, device=DEV, dtype=BF)  # [x | h'] rows
    x, before = buf[:, :K], buf.clone()
    acat = torch.randn(R, K, device=DEV, dtype=BF) * 0.05
    seed, offset, hscale = 1234, 8, 0.5
    res = C.lora_small_down(x, acat, p, seed, offset, p > 0, h_out=buf[:, K:], hscale=hscale)
    assert res
    xd = C.dropout_fwd_seeded(x.contiguous(), p, seed, offset) if p > 0 else x
    if p > 0:
        assert torch.equal(res[1], xd)
    _check(buf[:, K:], (xd.float() @ acat.float().t()) * hscale, f"down R{R} M{M} K{K} p{p}")
    assert torch.equal(buf[:, :K], before[:, :K])


@pytest.mark.parametrize("R", [8, 24])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dx(R, p):
    torch.manual_seed(5)
    C = _C()
    M, K, seed, offset = 100, 256, 77, 4
    g = torch.randn(M, R, device=DEV, dtype=BF)
    a = torch.randn(R, K, device=DEV, dtype=BF) * 0.1
    dx = torch.randn(M, K, device=DEV, dtype=BF)
    keep = (C.dropout_fwd_seeded(torch.ones(M, K, device=DEV, dtype=BF), p, seed, offset) != 0).float() if p > 0 else 1.0
    ref = dx.float() + keep * (g.float() @ a.float()) / (1 - p)
    assert C.lora_small_dx(g, a.t().contiguous(), dx, p, seed, offset, True)
    _check(dx, ref, f"dx R{R} p{p}")


def _lora_llama(r, p):
    from gke_ray_train_amd.models import build_llama
    from gke_ray_train_amd.peft import LoraConfig, get_peft_model
    torch.manual_seed(0)
    m = build_llama("llama-tiny-gqa", device=DEV, dtype=BF, seed=2)
    pm = get_peft_model(m, LoraConfig(r=r, lora_alpha=16, lora_dropout=p))
    for lm in pm.lora_modules.values():
        for b in lm.lora_B.values():
            torch.nn.init.normal_(b, 0, 0.02, generator=torch.Generator(device=DEV).manual_seed(9))
    ids = torch.randint(0, m.config.vocab_size, (2, 256), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    return pm, ids


@pytest.mark.parametrize("r", [8, 16])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_model_grads_kernels_vs_library(monkeypatch, r, p):
    """Adapter gradients of a LoRA Llama through DDP on the K-concatenated form and the small-rank
    kernels vs the epilogue form on library GEMMs: same loss, gradients within bf16."""
    import gke_ray_train_amd.peft.lora as L
    from gke_ray_train_amd.parallel import DistributedDataParallel
    res = {}
    for on in (True, False):
        monkeypatch.setattr(L, "_LORA_GRAD_KERNELS", on)
        monkeypatch.setattr(L, "_LORA_KCAT", on)
        pm, ids = _lora_llama(r, p)
        ddp = DistributedDataParallel(pm)
        torch.manual_seed(5)  # same dropout seeds both runs
        loss = pm(ids, labels=ids)["loss"]
        loss.backward()
        ddp.finish_gradient_sync()
        res[on] = (float(loss.detach()), {i: b.float().clone() for i, b in enumerate(ddp.grad_buffers())})
        if on:  # the attention projections of this model have kernel-sized widths: they took the hot path
            hot = [lm for n, lm in pm.lora_modules.items() if "attn" in n]
            assert hot and all(lm.kcat_pad > 0 and lm._bt is not None for lm in hot)
    (l1, g1), (l0, g0) = res[True], res[False]
    assert abs(l1 - l0) < 1e-3 * max(1.0, abs(l0))
    assert g1.keys() == g0.keys() and g1
    for n in g0:
        rel = (g1[n] - g0[n]).norm() / g0[n].norm().clamp_min(1e-8)
        assert rel < 2e-2, f"{n}: rel {rel.item():.3g}"


def test_rank4_trains():
    pm, ids = _lora_llama(4, 0.1)
    pm(ids, labels=ids)["loss"].backward()
    grads = [q.grad for q in pm.trainable_parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
