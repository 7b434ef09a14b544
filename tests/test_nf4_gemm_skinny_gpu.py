"""Skinny MFMA GEMM from NF4 codes (csrc/kernels/gemm_nf4_skinny.hip) for the 5-16 rows of a batched
decode step: the binding against float64 on the exact NF4 weight, its LoRA epilogue, bitwise
stability and refusals, the ``decode_step`` routing and batched generation from a 4-bit base.

Bound (derived, not measured): that of tests/test_nf4_gemv_gpu.py plus 2^-9 sum|x w| for the RNE
rounding of each level to bf16 (relative error <= 2^-9 per weight):
|y - y64| <= 2^-7 |y64| + (2^-9 + (terms + 64) 2^-24) sum|x w|."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_nf4_gemv_gpu as base  # noqa: E402  (_weights, _x, _lora_case, _check, _qlora_model, ...)

pytestmark = pytest.mark.gpu
DEV, SCALING = base.DEV, base.SCALING


def _skinny():
    return base._C().nf4_gemm_skinny


@pytest.mark.parametrize("M,N,K,strided", [
    (5, 20, 64, False),      # one block, partial second tile
    (9, 20, 192, True),      # blocks do not divide among the waves
    (16, 16, 2112, False),   # full A tile, K-loop tail
    (7, 768, 256, True),     # regular mid-size case
    (16, 64, 8192, False),   # Llama-size row, widest K split
    (6, 12, 4160, True),     # other K-split branch, with a tail
])
def test_kernel_matches_float64(M, N, K, strided):
    g = base._gen(1000 * M + N + K)
    q, a, w32 = base._weights(N, K, g)
    x = base._x(M, K, g, strided)
    y = _skinny()(x, q, a, N, K)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    base._check(y, y64, mag, K, f"nf4_gemm_skinny {M}x{N}x{K}", extra=2.0 ** -9 * mag)


@pytest.mark.parametrize("M,N,K,r,spans", [
    (8, 768, 256, 64, [(0, 512), (512, 128), (640, 128)]),   # three targets covering every row, two epilogue MFMAs
    (5, 768, 256, 16, [(0, 256), (512, 256)]),               # the middle 256 rows bare, lanes past r feed zeros
    (16, 20, 192, 8, [(0, 20)]),                             # one target, partial tile
    (12, 64, 8192, 8, [(4, 30)]),                            # target starts and ends inside a tile, widest K split
])
def test_lora_epilogue_matches_float64(M, N, K, r, spans):
    g = base._gen(7 * N + K + r)
    x, q, a, h, Bs, offs, y64, mag, lmag = base._lora_case(M, N, K, r, spans, g)
    y = _skinny()(x, q, a, N, K, h, Bs, offs, SCALING)
    base._check(y, y64, mag + lmag, K + r, f"nf4_gemm_skinny+lora {M}x{N}x{K} r={r}", extra=2.0 ** -9 * mag)
    if len(spans) > 1:  # the h column blocks follow the list order, not the row order
        perm = list(reversed(range(len(spans))))
        hp = torch.cat([h[:, i * r:(i + 1) * r] for i in perm], 1).contiguous()
        yp = _skinny()(x, q, a, N, K, hp, [Bs[i] for i in perm], [offs[i] for i in perm], SCALING)
        assert torch.equal(y, yp)


def test_bitwise_stable_and_refusals():
    C, f = base._C(), _skinny()
    g = base._gen(3)
    x, q, a, h, Bs, offs, *_ = base._lora_case(8, 768, 256, 16, [(0, 256), (512, 256)], g)
    q2, a2, _ = base._weights(64, 8192, g)
    x2 = base._x(16, 8192, g, False)
    first, second = [(f(x, q, a, 768, 256, h, Bs, offs, SCALING), f(x2, q2, a2, 64, 8192)) for _ in range(2)]
    assert all(torch.equal(u, v) for u, v in zip(first, second)), "two calls differ"
    with pytest.raises(RuntimeError, match="rows"):
        f(base._x(17, 256, g, False), q, a, 768, 256)
    q96, a96 = torch.zeros(16 * 96 // 2, device=DEV, dtype=torch.uint8), torch.ones(16 * 96 // 64, device=DEV)
    with pytest.raises(RuntimeError, match="K % 64"):
        f(base._x(8, 96, g, False), q96, a96, 16, 96)
    with pytest.raises(RuntimeError, match="bf16"):
        f(x.float(), q, a, 768, 256)
    for qq, aa in ((q, a[:-1].contiguous()), (q[:-1].contiguous(), a)):
        with pytest.raises(RuntimeError, match="shapes"):
            f(x, qq, aa, 768, 256)
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    for pat in (base.QNAN, 0):
        C.lds_fill(pat, torch.cuda.current_device())
        ya = f(x, q, a, 768, 256, h, Bs, offs, SCALING)
        C.lds_fill(pat, torch.cuda.current_device())
        yb = f(x2, q2, a2, 64, 8192)
        assert torch.equal(ya, first[0]) and torch.equal(yb, first[1]), f"stale LDS read (pattern {pat:#x})"


def test_batched_decode_never_dequantises(monkeypatch):
    """The test that fails without the feature: with the dequant cache off, a decode step of 8
    sequences used to dequantise every projection of every layer."""
    from gke_ray_train_amd.models.generation import GraphDecoder, KVCache, forward_cached
    from gke_ray_train_amd.peft.quant import NF4Linear
    pm = base._qlora_model("llama-tiny-gqa", "0", intermediate_size=1536)
    model = pm.base_model
    ids = torch.randint(0, 512, (8, 40), device=DEV, generator=base._gen(61))
    dec = GraphDecoder(model, 8, 64)
    logits = dec.prefill(ids)
    cache = KVCache(model.config, 8, 64, ids.device, torch.bfloat16)
    elogits = forward_cached(model, ids, cache)
    count = {"n": 0}
    for name in ("_dequant", "dequantize_into", "_dequant_t"):
        real = getattr(NF4Linear, name)

        def counted(self, *a, _real=real, **k):
            count["n"] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(NF4Linear, name, counted)
    for _ in range(8):
        logits = dec.step(logits.argmax(-1))
    torch.cuda.synchronize()
    assert count["n"] == 0, f"{count['n']} dequantisations in 8 graph decode steps of 8 rows"
    for _ in range(8):
        elogits = forward_cached(model, elogits.argmax(-1)[:, None], cache)
    assert count["n"] == 0, f"{count['n']} dequantisations in 8 eager decode steps of 8 rows"
    # outside a declared decode step 8 rows are the dequantising path, bit for bit
    g = base._gen(60)
    lin = base._nf4_linear(512, 256, False, g)
    lw = base._lora_on(lin, [(0, 128), (128, 128)], 8, g)
    x = base._x(8, 512, g, False)
    with torch.no_grad():
        assert torch.equal(lin(x), base._old_nf4(lin, x)) and torch.equal(lw(x), base._old_lora(lw, x))
    assert count["n"] > 0


@pytest.mark.parametrize("name,inter", [("llama-tiny-gqa", 1536), ("llama-tiny-d64", 768)])
@pytest.mark.parametrize("padded", [False, True])
def test_generate_batch_of_8_from_nf4_base(name, inter, padded):
    pm = base._qlora_model(name, None, intermediate_size=inter)
    P, T = 40, 8
    ids = torch.randint(0, 512, (8, P), device=DEV, generator=base._gen(7))
    lens = [40, 33, 25, 40, 17, 38, 29, 9] if padded else [P] * 8
    mask = torch.arange(P, device=DEV)[None, :] >= P - torch.tensor(lens, device=DEV)[:, None]
    kw = dict(attention_mask=mask.long()) if padded else {}
    out = pm.generate(ids, max_new_tokens=T, use_graph=True, **kw)
    eager = pm.generate(ids, max_new_tokens=T, use_graph=False, **kw)
    assert out.shape == (8, P + T) and torch.equal(out[:, :P], ids)
    assert torch.equal(out, eager), (out[:, P:], eager[:, P:])
    # teacher-forced per row, unpadded: the full recompute (dequantising path) ranks every token near the top
    for b, n in enumerate(lens):
        with torch.no_grad():
            lg = pm(out[b:b + 1, P - n:-1], return_logits=True)["logits"][0, n - 1:].float()
        best = lg.max(-1).values
        got = lg.gather(-1, out[b, P:, None]).squeeze(-1)
        assert bool((got >= best - (0.02 + 0.01 * best.abs())).all()), (b, (best - got).max().item())
