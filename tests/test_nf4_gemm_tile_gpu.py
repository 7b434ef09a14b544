"""Tile MFMA GEMM from NF4 codes (csrc/kernels/gemm_nf4_tile.hip) for the 17-256 rows of a prefill
chunk: the binding against float64 on the exact NF4 weight, its LoRA epilogue, bitwise stability
and refusals, the ``prefill_step`` routing and chunked-prefill generation from a 4-bit base.

Bound (derived, not measured): that of tests/test_nf4_gemm_skinny_gpu.py, which holds for any
summation order and so covers the K split:
|y - y64| <= 2^-7 |y64| + (2^-9 + (terms + 64) 2^-24) sum|x w|."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_nf4_gemv_gpu as base  # noqa: E402  (_weights, _x, _lora_case, _check, _qlora_model, ...)

pytestmark = pytest.mark.gpu
DEV, SCALING = base.DEV, base.SCALING


def _tile():
    return base._C().nf4_gemm_tile


@pytest.mark.parametrize("M,N,K,strided,k_split", [
    (17, 20, 64, False, 1),      # one block, partial wave, partial M tile
    (33, 130, 192, True, 1),     # second M tile with one row; N crosses the wave and the tile boundary; odd blocks
    (64, 128, 2112, False, 1),   # full tiles, K tail that is no whole step
    (128, 160, 256, True, 1),    # widest MT
    (129, 96, 512, False, 1),    # second row pass with one row
    (256, 64, 4160, False, 0),   # most rows, host-chosen split
    (40, 256, 1024, False, 3),   # uneven split, reduce kernel
    (20, 32, 8192, False, 0),    # long row
])
def test_kernel_matches_float64(M, N, K, strided, k_split):
    g = base._gen(1000 * M + N + K)
    q, a, w32 = base._weights(N, K, g)
    x = base._x(M, K, g, strided)
    y = _tile()(x, q, a, N, K, k_split=k_split)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y64 = x.double() @ w32.double().t()
    mag = x.double().abs() @ w32.double().abs().t()
    base._check(y, y64, mag, K, f"nf4_gemm_tile {M}x{N}x{K} split {k_split}", extra=2.0 ** -9 * mag)


@pytest.mark.parametrize("M,k_split", [(24, 1), (70, 2)])
@pytest.mark.parametrize("N,K,r,spans", [
    (768, 256, 64, [(0, 512), (512, 128), (640, 128)]),   # three targets covering every row, four epilogue MFMAs
    (768, 256, 16, [(0, 256), (512, 256)]),               # the middle 256 rows bare
    (20, 192, 8, [(0, 20)]),                              # one target, partial tile, lanes past r feed zeros
    (64, 8192, 8, [(4, 30)]),                             # target starts and ends inside a wave's 32 rows
])
def test_lora_epilogue_matches_float64(M, k_split, N, K, r, spans):
    g = base._gen(7 * N + K + r + M)
    x, q, a, h, Bs, offs, y64, mag, lmag = base._lora_case(M, N, K, r, spans, g)
    y = _tile()(x, q, a, N, K, h, Bs, offs, SCALING, k_split)
    base._check(y, y64, mag + lmag, K + r, f"nf4_gemm_tile+lora {M}x{N}x{K} r={r}", extra=2.0 ** -9 * mag)
    if len(spans) > 1:  # the h column blocks follow the list order, not the row order
        perm = list(reversed(range(len(spans))))
        hp = torch.cat([h[:, i * r:(i + 1) * r] for i in perm], 1).contiguous()
        yp = _tile()(x, q, a, N, K, hp, [Bs[i] for i in perm], [offs[i] for i in perm], SCALING, k_split)
        assert torch.equal(y, yp)


def test_bitwise_stable_and_refusals():
    C, f = base._C(), _tile()
    g = base._gen(3)
    x, q, a, h, Bs, offs, *_ = base._lora_case(40, 768, 256, 16, [(0, 256), (512, 256)], g)
    q2, a2, _ = base._weights(64, 8192, g)
    x2 = base._x(130, 8192, g, False)

    def run():
        return f(x, q, a, 768, 256, h, Bs, offs, SCALING), f(x2, q2, a2, 64, 8192, k_split=5)

    first, second = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(first, second)), "two calls differ"
    with pytest.raises(RuntimeError, match="rows"):
        f(base._x(257, 256, g, False), q, a, 768, 256)
    q96, a96 = torch.zeros(16 * 96 // 2, device=DEV, dtype=torch.uint8), torch.ones(16 * 96 // 64, device=DEV)
    with pytest.raises(RuntimeError, match="K % 64"):
        f(base._x(20, 96, g, False), q96, a96, 16, 96)
    with pytest.raises(RuntimeError, match="bf16"):
        f(x.float(), q, a, 768, 256)
    for qq, aa in ((q, a[:-1].contiguous()), (q[:-1].contiguous(), a)):
        with pytest.raises(RuntimeError, match="shapes"):
            f(x, qq, aa, 768, 256)
    with pytest.raises(RuntimeError, match="k_split"):  # 4 blocks in 3 splits of 2: the third is empty
        f(x, q, a, 768, 256, k_split=3)
    if not hasattr(C, "lds_fill"):
        pytest.skip("extension built without lds_fill")
    for pat in (base.QNAN, 0):
        C.lds_fill(pat, torch.cuda.current_device())
        ya = f(x, q, a, 768, 256, h, Bs, offs, SCALING)
        C.lds_fill(pat, torch.cuda.current_device())
        yb = f(x2, q2, a2, 64, 8192, k_split=5)
        assert torch.equal(ya, first[0]) and torch.equal(yb, first[1]), f"stale LDS read (pattern {pat:#x})"


def test_prefill_never_dequantises(monkeypatch):
    """The test that fails without the feature: with the dequant cache off, every prefill chunk of
    more than 16 rows used to dequantise every projection of every layer."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.models.generation import GraphDecoder, KVCache, forward_cached
    from gke_ray_train_amd.peft import quant
    from gke_ray_train_amd.peft.quant import NF4Linear
    monkeypatch.setattr(quant, "NF4_TILE_MAX_ROWS", quant.NF4_TILE_KERNEL_ROWS)
    pm = base._qlora_model("llama-tiny-gqa", "0", intermediate_size=1536)
    model = pm.base_model
    ids = torch.randint(0, 512, (1, 40), device=DEV, generator=base._gen(61))
    count = {"n": 0}
    for name in ("_dequant", "dequantize_into", "_dequant_t"):
        real = getattr(NF4Linear, name)

        def counted(self, *a, _real=real, **k):
            count["n"] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(NF4Linear, name, counted)
    cache = KVCache(model.config, 1, 64, ids.device, torch.bfloat16)
    elogits = forward_cached(model, ids, cache)
    assert count["n"] == 0, f"{count['n']} dequantisations in a 40-row prefill"
    dec = GraphDecoder(model, 1, 64)
    logits = dec.prefill(ids, prefill_chunk_size=24)
    assert count["n"] == 0, f"{count['n']} dequantisations in a prefill in chunks of 24 and 16 rows"
    for _ in range(8):
        logits = dec.step(logits.argmax(-1))
        elogits = forward_cached(model, elogits.argmax(-1)[:, None], cache)
    torch.cuda.synchronize()
    assert count["n"] == 0, f"{count['n']} dequantisations in 8 decode steps"
    assert torch.isfinite(logits).all() and torch.isfinite(elogits).all()
    # outside a declared prefill 40 rows are the dequantising path, bit for bit
    g = base._gen(60)
    lin = base._nf4_linear(512, 256, False, g)
    lw = base._lora_on(lin, [(0, 128), (128, 128)], 8, g)
    x = base._x(40, 512, g, False)
    with torch.no_grad():
        assert torch.equal(lin(x), base._old_nf4(lin, x)) and torch.equal(lw(x), base._old_lora(lw, x))
    assert count["n"] > 0
    # with the cache on a declared prefill stays on the resident W
    quant.set_dequant_cache(model, "1")
    calls = []
    monkeypatch.setattr(ops, "nf4_gemm_tile", lambda *a, **k: calls.append(1))
    forward_cached(model, ids, KVCache(model.config, 1, 64, ids.device, torch.bfloat16))
    assert not calls


@pytest.mark.parametrize("name,inter", [("llama-tiny-gqa", 1536), ("llama-tiny-d64", 768)])
def test_generate_with_chunked_prefill_from_nf4_base(name, inter, monkeypatch):
    from gke_ray_train_amd.peft import quant
    monkeypatch.setattr(quant, "NF4_TILE_MAX_ROWS", quant.NF4_TILE_KERNEL_ROWS)
    pm = base._qlora_model(name, "0", intermediate_size=inter)
    P, T = 40, 8
    ids = torch.randint(0, 512, (2, P), device=DEV, generator=base._gen(7))
    out = pm.generate(ids, max_new_tokens=T, use_graph=True, prefill_chunk_size=12)  # 24 rows per chunk
    eager = pm.generate(ids, max_new_tokens=T, use_graph=False, prefill_chunk_size=12)
    assert out.shape == (2, P + T) and torch.equal(out[:, :P], ids)
    assert torch.equal(out, eager), (out[:, P:], eager[:, P:])
    # teacher-forced: the full recompute (dequantising path) ranks every generated token near the top
    with torch.no_grad():
        lg = pm(out[:, :-1], return_logits=True)["logits"][:, P - 1:].float()
    best = lg.max(-1).values
    got = lg.gather(-1, out[:, P:].unsqueeze(-1)).squeeze(-1)
    assert bool((got >= best - (0.02 + 0.01 * best.abs())).all()), (best - got).max().item()
