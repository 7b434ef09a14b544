"""``ops.nf4_gemv`` on CPU tensors (the ``_ref`` path) against the float64 formula on the exact NF4
weight, and ``NF4Linear`` / ``LoraLinear`` on CPU: the decode branches are GPU-only and leave the CPU
forward as it was."""
import pytest
import torch
import torch.nn.functional as F

from gke_ray_train_amd import ops
from gke_ray_train_amd.ops import _ref
from gke_ray_train_amd.peft.lora import LoraConfig, LoraLinear
from gke_ray_train_amd.peft.quant import BitsAndBytesConfig, NF4Linear

SCALING = 1.75


def _weights(N, K, g):
    w = torch.randn(N * K // 64, 64, generator=g) * torch.exp2(torch.rand(N * K // 64, 1, generator=g) * 12 - 6)
    q, a = ops.nf4_quantize(w.view(-1), 64)
    return q, a, _ref.nf4_dequantize(q, a, N * K, 64, torch.float32).view(N, K)


def _bound(y64, mag, terms):
    return 2.0 ** -7 * y64.abs() + (terms + 64) * 2.0 ** -24 * mag


@pytest.mark.parametrize("M,N,K", [(1, 4, 64), (3, 20, 192), (4, 20, 2112), (2, 768, 256)])
def test_cpu_op_matches_float64(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    q, a, w32 = _weights(N, K, g)
    x = torch.randn(M, K, generator=g).bfloat16()
    y = ops.nf4_gemv(x, q, a, N, K)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    assert bool(((y.double() - y64).abs() <= _bound(y64, mag, K)).all())


@pytest.mark.parametrize("M,N,K,r,spans", [
    (2, 768, 256, 64, [(0, 512), (512, 128), (640, 128)]),
    (3, 768, 256, 16, [(0, 256), (512, 256)]),
    (1, 20, 192, 8, [(0, 20)]),
])
def test_cpu_op_lora_epilogue_matches_float64(M, N, K, r, spans):
    g = torch.Generator().manual_seed(N + K + r)
    q, a, w32 = _weights(N, K, g)
    x = torch.randn(M, K, generator=g).bfloat16()
    h = torch.randn(M, r * len(spans), generator=g).bfloat16()
    Bs = [(torch.randn(n, r, generator=g) * 0.05).bfloat16() for _, n in spans]
    y = ops.nf4_gemv(x, q, a, N, K, h, Bs, [off for off, _ in spans], SCALING)
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    for i, ((off, n), b) in enumerate(zip(spans, Bs)):
        hi = h[:, i * r:(i + 1) * r].double()
        y64[:, off:off + n] += SCALING * (hi @ b.double().t())
        mag[:, off:off + n] += SCALING * (hi.abs() @ b.double().abs().t())
    assert bool(((y.double() - y64).abs() <= _bound(y64, mag, K + r)).all())
    bare = torch.ones(N, dtype=torch.bool)
    for off, n in spans:
        bare[off:off + n] = False
    assert torch.equal(y[:, bare], ops.nf4_gemv(x, q, a, N, K)[:, bare])  # rows outside every target: no adapter term


@pytest.mark.parametrize("double_quant", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 5])
def test_cpu_modules_unchanged(double_quant, rows, monkeypatch):
    """Kernel-sized inputs under no_grad on CPU: NF4Linear is F.linear on the dequantised weight and
    LoraLinear is the base output plus the block-placed adapter term, and neither calls the GEMV."""
    calls = []
    monkeypatch.setattr(ops, "nf4_gemv", lambda *a, **k: calls.append(1))
    g = torch.Generator().manual_seed(10 + rows)
    K, N, r = 128, 64, 8
    lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) * 0.05)
    base = NF4Linear.from_linear(lin, BitsAndBytesConfig(bnb_4bit_use_double_quant=double_quant)).eval()
    spans = [(0, 32), (40, 24)]
    lw = LoraLinear(base, [(f"t{i}_proj", off, n) for i, (off, n) in enumerate(spans)],
                    LoraConfig(r=r, lora_alpha=14, lora_dropout=0.1)).eval()
    with torch.no_grad():
        for p in lw.lora_B.values():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    x = torch.randn(rows, K, generator=g).bfloat16()
    with torch.no_grad():
        y, yl = base(x), lw(x)
        want = F.linear(x, base.dequantize())
        assert torch.equal(y, want)
        add = torch.zeros_like(want)
        bfull = torch.zeros(N, r * len(spans), dtype=torch.bfloat16)
        for i, (off, n) in enumerate(spans):
            bfull[off:off + n, i * r:(i + 1) * r] = lw.lora_B[f"t{i}_proj"]
        a = torch.cat([lw.lora_A[f"t{i}_proj"] for i in range(len(spans))], 0)
        add = F.linear(F.linear(x, a) * lw.scaling, bfull)
        assert torch.equal(yl, want + add)
    assert not calls
    assert not hasattr(base, "_absmax_cache")
