"""KV-cache generation for the Llama family (greedy / sampling).

Reference role: ``model.generate(**inputs, max_new_tokens=..., do_sample=False,
eos_token_id=[eos, <|eot_id|>])`` in the post-training comparison (ray-jobs/fine_tune_llama_ray.py:
138-146). The cache is one preallocated [B, S_max, Hkv, D] K and V tensor per
layer (sized for prompt + max_new_tokens up front, no re-allocation while decoding); prefill and
every decode step run the SAME flash-attention kernel over a strided view of the cache
(bottom-right-aligned causal mask, Sq = new tokens, Sk = tokens so far) with RoPE applied at the
absolute positions by the RoPE kernel's position array.

On MI355X the one-token decode step is launch-bound (≈10 kernels per layer, a few µs of work
each), so ``GraphDecoder`` captures the WHOLE step — embedding, every layer, final norm, LM head
and, when it is given a ``SamplerConfig``, the choice of the token — into one HIP graph and replays
it per token. Everything that changes between tokens lives in device tensors the graph reads: the
current position (one per row: RoPE position and KV-cache slot) and the per-row valid key
length, which the flash kernel takes as its padding mask (``seqlens_k``) over the full-length
cache, so the kernel's tile loop still covers only the keys written so far.

Both are per batch row, which is what a padded batch (``attention_mask``) uses: the prompts are
compacted to column 0 and prefilled as one causal [B, longest] block, each row's logits are taken
at its own last token, and row b then decodes at position len_b + t into cache slot len_b + t
(over the K / V the prefill left there for the filler behind a short row) with len_b + t + 1 valid
keys. No kernel knows about padding.

With a sampler the step ends in ``sample_logits`` (csrc/kernels/sample.hip): greedy argmax or a
temperature / top-k / top-p draw with counter-based noise, plus the loop's bookkeeping (pad after
EOS, finished flags, the next step's input id, the output column), so ``generate()`` is
back-to-back replays with no torch op between them and one host read of ``finished.all()`` every
``sync_every`` tokens; the output is trimmed to HF's stopping point. ``GRT_DEVICE_SAMPLER=0`` (or
``device_loop=False``) restores the host loop, which picks the token with torch ops on the logits
the graph returns. ``ops/_ref.py::sample_tokens`` is the sampler's host implementation: the same
logits, seed and counter give the same token on either device.

Prompt-lookup speculative decoding (``generate(..., prompt_lookup_num_tokens=K)``, one sequence)
replaces the one-token step by a VERIFY step of T = K + 1 tokens: the last emitted token, not yet
in the cache, and K drafts copied from where the last n-gram occurred before in the prompt and the
tokens so far. It is the same captured step with T rows (one position per token; split-K decode
attention in which token t sees the keys up to its own) and another tail: the sampler's candidate
mode and ``spec_advance`` (see ``GraphDecoder``), so the loop is still graph replays and one host
read per ``sync_every`` of them. The slots of rejected drafts lie past the valid length and are
rewritten by the next step; a finished or full row is inert. ``ops/_ref.py::prompt_lookup_draft``
and ``::spec_accept`` are the host implementations, which the host loops (``device_loop=False``,
``use_graph=False``) run on the logits [T, V] of the same step.

fp8 KV cache (``generate(..., kv_cache_dtype="fp8")``, ``KVCache(..., "fp8")``): K and V are stored
as OCP e4m3fn codes with one fp32 scale per (token, kv head) (``ops/_ref.py::kv_fp8_quantize`` is
the definition), (D + 4) / 2D of the bf16 cache's bytes. ``rope_append_fp8`` (kv_fp8.hip) rotates
K, rounds it to bf16 (the value the bf16 cache would hold) and quantises it and V on the way in;
the split-K decode kernel reads the codes directly (``ops.decode_attention_fp8``, T = 1..4 tokens).
The prefill of an empty cache fills the cache the same way but attends over the fresh bf16 K / V,
so its logits are bitwise those of the bf16 cache. DECODE TOKENS ATTEND TO THEIR OWN K / V AS
STORED, that is, quantised: a token's key and value are written before its attention runs, and
the kernel reads nothing but the cache. In the captured one-token step the qkv GEMV runs without
its RoPE / append epilogue and ``rope_append_fp8`` follows it: one launch per layer more than the
bf16 step. A chunk of more than 4 tokens on a non-empty cache (chunked prefill) is a slow path:
append, dequantise rows [0, n) to bf16 (``kv_fp8_dequant``) and run the flash kernel. Without the
HIP kernels (CPU, fp32 model, other head dims) the cache is quantised by ``_ref`` and attention
runs over the dequantised rows. There is no flash-kernel decode path for the fp8 cache:
``GRT_DECODE_ATTN=0`` with it is refused wherever it would run on those kernels.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import torch

from .. import _native, ops
from ..ops import _ref


KV_CACHE_DTYPES = (None, "auto", "fp8", "fp8_e4m3")


def _kv_dtype(model, kv_cache_dtype):
    """``KVCache``'s dtype argument for a ``kv_cache_dtype`` choice: the model's dtype or "fp8"."""
    if kv_cache_dtype not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES}, got {kv_cache_dtype!r}")
    return "fp8" if kv_cache_dtype in ("fp8", "fp8_e4m3") else _cache_dtype(model)


def _fp8_kernels_ok(is_cuda: bool, dtype, D: int) -> bool:
    """The fp8 cache runs on the HIP kernels (``rope_append_fp8``, fp8 decode attention): a bf16 model
    on the GPU with head_dim 128 or 64. Anything else quantises with ``_ref``."""
    return is_cuda and dtype == torch.bfloat16 and D in (64, 128) and _native.kernels_available()


def _check_fp8_decode(fp8: bool, is_cuda: bool, dtype, D: int) -> None:
    """``GRT_DECODE_ATTN=0`` sends decode attention to the flash kernel, which cannot read fp8 codes:
    refused wherever the fp8 cache would run on the kernels (the ``_ref`` path has no such kernel)."""
    from ..ops import fused
    if fp8 and not fused._DECODE_KERNEL and _fp8_kernels_ok(is_cuda, dtype, D):
        raise ValueError("kv_cache_dtype='fp8' with GRT_DECODE_ATTN=0: the fp8 KV cache is read by the split-K decode "
                         "kernel only, there is no flash-kernel decode path for it")


class KVCache:
    """``dtype`` a torch dtype, or "fp8": k / v are then uint8 e4m3fn codes [B, max_len, Hkv, D] and
    ``k_scale`` / ``v_scale`` hold one fp32 scale per (row, slot, kv head) (see module doc)."""

    def __init__(self, cfg, B, max_len, device, dtype):
        hd, hkv = cfg.head_dim, cfg.num_key_value_heads
        self.fp8 = isinstance(dtype, str)
        if self.fp8:
            if dtype not in ("fp8", "fp8_e4m3"):
                raise ValueError(f"KVCache: dtype must be a torch dtype or 'fp8', got {dtype!r}")
            dtype = torch.uint8
            self.k_scale, self.v_scale = ([torch.zeros(B, max_len, hkv, device=device, dtype=torch.float32)
                                           for _ in range(cfg.num_hidden_layers)] for _ in range(2))
        self.k = [torch.zeros(B, max_len, hkv, hd, device=device, dtype=dtype) for _ in range(cfg.num_hidden_layers)]
        self.v = [torch.zeros(B, max_len, hkv, hd, device=device, dtype=dtype) for _ in range(cfg.num_hidden_layers)]
        self.len = 0
        self.max_len = max_len
        # per-row token counts [B] int32 after a masked (ragged) prefill; ``len`` is then the longest
        # row's, which is what the fullness checks compare with ``max_len``
        self.lens: Optional[torch.Tensor] = None

    def nbytes(self) -> int:
        """Bytes held by the cache tensors (codes and scales of an fp8 cache)."""
        ts = self.k + self.v + ((self.k_scale + self.v_scale) if self.fp8 else [])
        return sum(t.numel() * t.element_size() for t in ts)


@dataclass
class _MaskRows:
    """A non-trivial attention mask, read on the host: row b's tokens are the columns
    ``start[b] ... start[b] + lens[b] - 1`` of the padded batch."""
    start: List[int]
    lens: List[int]


def _mask_rows(attention_mask, B: int, S: int) -> Optional[_MaskRows]:
    """Validate an HF-style ``attention_mask`` [B, S] (bool / integer, any device; one host read):
    each row's ones must be one contiguous run of at least one token, with the padding on the left,
    on the right or on both sides. ``None`` for no mask or an all-ones mask (nothing to do)."""
    if attention_mask is None or isinstance(attention_mask, _MaskRows):
        return attention_mask
    m = torch.as_tensor(attention_mask)
    if tuple(m.shape) != (B, S):
        raise ValueError(f"attention_mask has shape {tuple(m.shape)}, input_ids has {(B, S)}")
    m = (m != 0).cpu()
    if bool(m.all()):
        return None
    lens = m.sum(1).tolist()
    start = m.int().argmax(1).tolist()
    for b, (a, n) in enumerate(zip(start, lens)):
        if n == 0:
            raise ValueError(f"attention_mask row {b} is all zeros: every row needs at least one token")
        if not bool(m[b, a:a + n].all()):
            raise ValueError(f"attention_mask row {b} has a hole: its ones must form one contiguous run")
    return _MaskRows(start, lens)


def _compact(ids: torch.Tensor, rows: _MaskRows) -> torch.Tensor:
    """Row b's masked tokens moved to columns 0 ... lens[b] - 1 of a [B, max lens] block; the
    filler behind a short row is id 0, whatever the pad columns held."""
    j = torch.arange(max(rows.lens), device=ids.device)[None, :]
    start = torch.tensor(rows.start, device=ids.device)[:, None]
    lens = torch.tensor(rows.lens, device=ids.device)[:, None]
    picked = ids.gather(1, (start + j).clamp_(max=ids.shape[1] - 1))
    return torch.where(j < lens, picked, torch.zeros_like(picked))


def _row_prompt(input_ids: torch.Tensor, rows: Optional[_MaskRows]) -> torch.Tensor:
    """The masked tokens [n] of a batch of one row."""
    return input_ids[0] if rows is None else input_ids[0, rows.start[0]:rows.start[0] + rows.lens[0]]


def _cache_dtype(model) -> torch.dtype:
    dt = next(model.parameters()).dtype
    return dt if dt in (torch.bfloat16, torch.float32) else torch.bfloat16


def _layers(model, h, attend):
    """The layer skeleton of every cached step (norm, qkv, attention, o_proj, norm, MLP) over all
    layers, then the final norm. ``attend(li, attn, qkv)`` is the RoPE / cache-append / attention
    middle of layer ``li`` (``_eager_attention`` or ``_device_attention``); it returns
    o [rows, hq * D]."""
    residual = None
    for li, layer in enumerate(model.model.layers):
        attn = layer.self_attn
        eps = layer.input_layernorm.eps
        if residual is None:
            residual = h
            x = ops.rms_norm(h, layer.input_layernorm.weight, eps)
        else:
            x, residual = ops.add_rms_norm(h, residual, layer.input_layernorm.weight, eps)
        h = attn.o_proj(attend(li, attn, attn.qkv_proj(x)))
        x, residual = ops.add_rms_norm(h, residual, layer.post_attention_layernorm.weight, eps)
        h = _mlp(layer.mlp, x)
    return ops.add_rms_norm(h, residual, model.model.norm.weight, model.model.norm.eps)[0]


def _eager_attention(attn, qkv, B, S, pos0, cos, sin, cache: KVCache, li: int, row_pos=None):
    """``row_pos`` [B] int32: the one-token step of a ragged cache, row b's token at position and
    cache slot row_pos[b]; without it the S tokens of every row sit at pos0 ... pos0 + S - 1."""
    hq, hkv, D = attn.hq, attn.hkv, attn.hd
    pos = row_pos if row_pos is not None else torch.arange(pos0, pos0 + S, device=qkv.device, dtype=torch.int32).repeat(B)
    if cache.fp8:
        return _eager_attention_fp8(attn, qkv, B, S, pos0, cos, sin, cache, li, row_pos, pos)
    if _fused_ok(qkv, cache, li):
        # RoPE of q / k and the cache append of k / v in one kernel (rope_append, elementwise.hip)
        q = _native.kernels().rope_append(qkv.contiguous(), cos, sin, pos, hq, hkv, D, cos.shape[0],
                                          cache.k[li], cache.v[li], S)
    else:
        x3 = qkv.view(B * S, hq + 2 * hkv, D)
        q = _ref.apply_rope(x3[:, :hq], cos, sin, pos)
        k = _ref.apply_rope(x3[:, hq:hq + hkv], cos, sin, pos)
        v = qkv.view(B, S, hq + 2 * hkv, D)[:, :, hq + hkv:]
        if row_pos is None:
            cache.k[li][:, pos0:pos0 + S] = k.view(B, S, hkv, D)
            cache.v[li][:, pos0:pos0 + S] = v
        else:
            b = torch.arange(B, device=qkv.device)
            cache.k[li][b, row_pos.long()] = k.view(B, hkv, D)
            cache.v[li][b, row_pos.long()] = v[:, 0]
    kk = cache.k[li][:, :pos0 + S]
    vv = cache.v[li][:, :pos0 + S]
    if row_pos is None:
        o = ops.flash_attention(q.view(B, S, hq, D), kk, vv, causal=True)
    else:  # slots past a short row's own tokens hold the prefill's filler: masked by the valid length
        o = ops.flash_attention(q.view(B, 1, hq, D), kk, vv, causal=False, seqlens_k=row_pos + 1)
    return o.reshape(B * S, hq * D)


def _fp8_append(K, qkv, cos, sin, pos, hq, hkv, D, cache: KVCache, li: int, tpr: int, k_out=None):
    """q [M, hq, D] rotated; K (rotated, rounded to bf16) and V quantised into the fp8 cache."""
    return K.rope_append_fp8(qkv.contiguous(), cos, sin, pos, hq, hkv, D, cos.shape[0], cache.k[li], cache.v[li],
                             cache.k_scale[li], cache.v_scale[li], tpr, k_out=k_out)


def _eager_attention_fp8(attn, qkv, B, S, pos0, cos, sin, cache: KVCache, li: int, row_pos, pos):
    """``_eager_attention`` over an fp8 cache (see module doc): the prefill of an empty cache
    attends over the fresh unquantised K / V; every later call attends over the cache as stored."""
    hq, hkv, D = attn.hq, attn.hkv, attn.hd
    n = pos0 + S
    prefill = pos0 == 0 and row_pos is None
    lens = row_pos + 1 if row_pos is not None else None
    x4 = qkv.view(B, S, hq + 2 * hkv, D)
    if _fp8_kernels_ok(qkv.is_cuda, qkv.dtype, D):
        _check_fp8_decode(True, True, qkv.dtype, D)  # a direct forward_cached obeys the switch too
        K = _native.kernels()
        k_out = torch.empty(B * S, hkv, D, device=qkv.device, dtype=qkv.dtype) if prefill else None
        q = _fp8_append(K, qkv, cos, sin, pos, hq, hkv, D, cache, li, S, k_out).view(B, S, hq, D)
        if prefill:
            o = ops.flash_attention(q, k_out.view(B, S, hkv, D), x4[:, :, hq + hkv:], causal=True)
        elif S <= 4:
            o = ops.decode_attention_fp8(q, cache.k[li][:, :n], cache.v[li][:, :n], cache.k_scale[li][:, :n],
                                         cache.v_scale[li][:, :n], seqlens_k=lens)
        else:  # chunked prefill, the slow path: a bf16 copy of the rows so far for the flash kernel
            kk = K.kv_fp8_dequant(cache.k[li], cache.k_scale[li], n)
            vv = K.kv_fp8_dequant(cache.v[li], cache.v_scale[li], n)
            o = ops.flash_attention(q, kk, vv, causal=True)
        return o.reshape(B * S, hq * D)
    x3 = qkv.view(B * S, hq + 2 * hkv, D)
    q = _ref.apply_rope(x3[:, :hq], cos, sin, pos).view(B, S, hq, D)
    k = _ref.apply_rope(x3[:, hq:hq + hkv], cos, sin, pos).view(B, S, hkv, D)
    v = x4[:, :, hq + hkv:]
    (kq, ks), (vq, vs) = _ref.kv_fp8_quantize(k), _ref.kv_fp8_quantize(v)
    if row_pos is None:
        cache.k[li][:, pos0:n], cache.k_scale[li][:, pos0:n] = kq, ks
        cache.v[li][:, pos0:n], cache.v_scale[li][:, pos0:n] = vq, vs
    else:
        b, slot = torch.arange(B, device=qkv.device), row_pos.long()
        cache.k[li][b, slot], cache.k_scale[li][b, slot] = kq[:, 0], ks[:, 0]
        cache.v[li][b, slot], cache.v_scale[li][b, slot] = vq[:, 0], vs[:, 0]
    if prefill:
        kk, vv = k, v
    else:
        kk = _ref.kv_fp8_dequantize(cache.k[li][:, :n], cache.k_scale[li][:, :n], qkv.dtype)
        vv = _ref.kv_fp8_dequantize(cache.v[li][:, :n], cache.v_scale[li][:, :n], qkv.dtype)
    if row_pos is None:
        o = ops.flash_attention(q, kk, vv, causal=True)
    else:
        o = ops.flash_attention(q, kk, vv, causal=False, seqlens_k=lens)
    return o.reshape(B * S, hq * D)


def _device_attention(attn, qkv, B, T, cos, sin, cache: KVCache, li: int, pos_b, lens):
    """The captured step's middle, every position read from device tensors: T tokens per row at
    positions and cache slots pos_b [B * T] (rows differ after a masked prefill), the last T of the
    row's ``lens`` valid keys. ``T`` > 1 is the verify step of speculative decoding."""
    hq, hkv, D = attn.hq, attn.hkv, attn.hd
    if cache.fp8:
        q = _fp8_append(_native.kernels(), qkv, cos, sin, pos_b, hq, hkv, D, cache, li, T)
        o = ops.decode_attention_fp8(q.view(B, T, hq, D), cache.k[li], cache.v[li], cache.k_scale[li],
                                     cache.v_scale[li], seqlens_k=lens)
        return o.reshape(B * T, hq * D)
    q = _native.kernels().rope_append(qkv.contiguous(), cos, sin, pos_b, hq, hkv, D, cos.shape[0],
                                      cache.k[li], cache.v[li], T)
    if T == 1:
        o = ops.flash_attention(q.view(B, 1, hq, D), cache.k[li], cache.v[li], causal=False, seqlens_k=lens)
    else:
        o = ops.decode_attention_multi(q.view(B, T, hq, D), cache.k[li], cache.v[li], seqlens_k=lens)
    return o.reshape(B * T, hq * D)


def _fused_ok(qkv, cache: KVCache, li: int) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and cache.k[li].dtype == torch.bfloat16
            and qkv.shape[-1] % 8 == 0 and _native.kernels_available())


def _mlp(mlp, x):
    """Decode MLP: for 1-2 tokens (``GEMV_MAX_ROWS``) the down projection is a GEMV whose input
    SwiGLU is computed on the fly from the fused gate/up output (gemv.hip, one launch instead of
    SwiGLU + GEMV)."""
    from ..ops import linear as _lin
    down = mlp.down_proj
    if (_lin._GEMV and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[0] <= _lin.GEMV_MAX_ROWS
            and type(down) is _lin.Linear and down.bias is None and down.weight.dtype == torch.bfloat16
            and down.weight.is_contiguous() and down.in_features % 8 == 0 and not torch.is_grad_enabled()):
        gu = mlp.gate_up_proj(x)
        if gu.is_contiguous() and gu.data_ptr() % 16 == 0 and gu.shape[-1] == 2 * down.in_features:
            return _native.kernels().gemv(gu, down.weight, swiglu=True)
        return down(ops.swiglu(gu))
    return mlp(x)


@torch.no_grad()
def forward_cached(model, ids: torch.Tensor, cache: KVCache, attention_mask=None,
                   all_logits: bool = False) -> torch.Tensor:
    """Run `ids` [B, S] at positions cache.len ... ; returns last-position logits [B, V], or with
    ``all_logits`` those of every position [B, S, V] (the verify step of speculative decoding;
    not with a padded ``attention_mask``).

    With a non-trivial ``attention_mask`` [B, S] (prefill of an empty cache only) row b's prompt is
    its masked tokens at positions 0 ... len_b - 1: the rows are compacted to column 0 and run as one
    causal block, whose filler behind a short row comes after that row's tokens and so stays hidden
    from them; the logits are those of each row's last real token. The cache is ragged from then on
    (``cache.lens``): each later call takes one token per row, at position and cache slot len_b
    (over the filler's K / V), attending to that row's len_b + 1 keys."""
    B, S = ids.shape
    rows = _mask_rows(attention_mask, B, S)
    row_pos = None
    if rows is not None:
        if cache.len != 0:
            raise ValueError(f"forward_cached: an attention_mask with padding needs an empty cache (prefill), "
                             f"this one holds {cache.len} tokens")
        ids = _compact(ids, rows)
        S = ids.shape[1]
    elif cache.lens is not None:
        if S != 1:
            raise ValueError(f"forward_cached: a ragged cache takes one token per row and call, got {S}")
        row_pos = cache.lens
    pos0 = cache.len
    if pos0 + S > cache.max_len:  # rope_append writes no cache row past max_len: refuse, don't truncate
        raise ValueError(f"KV cache overflow: {pos0} cached + {S} new tokens > max_len {cache.max_len}")
    cos, sin = model.rope(cache.max_len, ids.device)
    h = model.model.embed_tokens(ids).view(B * S, -1)
    x = _layers(model, h, lambda li, attn, qkv: _eager_attention(attn, qkv, B, S, pos0, cos, sin, cache, li, row_pos))
    if all_logits:
        if rows is not None or row_pos is not None:
            raise ValueError("forward_cached: all_logits needs an unpadded, non-ragged cache")
        cache.len += S
        return model.lm_head(x).float().view(B, S, -1)
    if rows is not None:
        cache.lens = torch.tensor(rows.lens, dtype=torch.int32, device=ids.device)
        last = x.view(B, S, -1)[torch.arange(B, device=ids.device), cache.lens.long() - 1]
    else:
        last = x.view(B, S, -1)[:, -1]
        if row_pos is not None:
            cache.lens = row_pos + 1
    cache.len += S
    return model.lm_head(last).float()


_GEMV_NORM = os.environ.get("GRT_GEMV_NORM", "1") != "0"


def _plain_bf16_linear(lin) -> bool:
    from ..ops import linear as _lin
    w = getattr(lin, "weight", None)
    return (isinstance(lin, _lin.Linear) and type(lin).forward is _lin.Linear.forward and lin.bias is None
            and w.dtype == torch.bfloat16 and w.is_cuda and w.is_contiguous() and w.shape[1] % 8 == 0
            and w.data_ptr() % 16 == 0)


GEMV_FUSED_MAX_ROWS = 4  # gemv_fused's row limit (TORCH_CHECK in csrc/bindings/ops.cpp)


def _norm_fusable(model, B: int) -> bool:
    """Every projection a plain bf16 Linear (no LoRA / NF4 wrappers, no bias) and 1-2 rows: the
    decode step can run with its residual adds / RMSNorms inside the GEMVs (gemv.hip)."""
    from ..ops import linear as _lin
    if not (_GEMV_NORM and _lin._GEMV and B <= min(_lin.GEMV_MAX_ROWS, GEMV_FUSED_MAX_ROWS) and _native.kernels_available()):
        return False
    m = model.model
    norms = [m.norm] + [n for ly in m.layers for n in (ly.input_layernorm, ly.post_attention_layernorm)]
    lins = [model.lm_head] + [p for ly in m.layers for p in (ly.self_attn.qkv_proj, ly.self_attn.o_proj,
                                                               ly.mlp.gate_up_proj, ly.mlp.down_proj)]
    if model.config.head_dim not in (64, 128):  # the RoPE epilogue / decode attention kernels
        return False
    return (all(_plain_bf16_linear(p) for p in lins)
            and all(n.weight.dtype == torch.bfloat16 and n.weight.is_contiguous() and n.weight.data_ptr() % 16 == 0
                    for n in norms))


class _NormWorkspace:
    """Fixed-point sums of squares of the residual stream's rows (gemv.hip): two [B, 64] slots, the
    producer GEMVs (o_proj, down_proj) alternate between them and each zeroes the other for the
    next one. 2 producers per layer, so the slot sequence repeats every token (graph replay)."""

    def __init__(self, B: int, device):
        self.sumsq = torch.zeros(2, B, 64, dtype=torch.int64, device=device)


def _fused_norm_layer_step(layer, h, first: bool, ws: _NormWorkspace, B, cos, sin, cache: KVCache, li: int,
                           pos_b, lens):
    """One-token layer step with the residual adds, RMSNorms and RoPE inside the GEMVs: o_proj /
    down_proj write h = y + residual and add sum(h^2) to a fixed-point accumulator, qkv / gate_up
    normalise their input on the fly from (h, accumulator, norm weight), and the qkv epilogue
    rotates q / k and appends k / v to the cache. ``h`` IS the residual stream between
    layers; slot 0 carries the post-attention norm's statistics, slot 1 the next input norm's.
    With an fp8 cache the qkv GEMV has no epilogue (its norm-on-load stays) and ``rope_append_fp8``
    follows it, one more launch per layer; the fp8 decode kernel then reads the cache."""
    K = _native.kernels()
    attn, mlp = layer.self_attn, layer.mlp
    ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
    hq, hkv, D = attn.hq, attn.hkv, attn.hd
    # the qkv GEMV's epilogue applies RoPE and appends k / v to the cache (no rope_append launch)
    rope = {} if cache.fp8 else dict(cos=cos, sin=sin, pos=pos_b, kc=cache.k[li], vc=cache.v[li], hq=hq, hkv=hkv)
    if first and cache.fp8:  # no norm-on-load and no epilogue: the plain GEMV
        q = K.gemv(ops.rms_norm(h, ln1.weight, ln1.eps), attn.qkv_proj.weight)
    elif first:  # layer 0: h is the embedding (no residual add, no producer GEMV summed its squares)
        q = K.gemv_fused(ops.rms_norm(h, ln1.weight, ln1.eps), attn.qkv_proj.weight, ws.sumsq, 1, **rope)
    else:
        q = K.gemv_fused(h, attn.qkv_proj.weight, ws.sumsq, 1, g=ln1.weight, eps=ln1.eps, **rope)
    if cache.fp8:  # q is the whole qkv row here
        q = _fp8_append(K, q, cos, sin, pos_b, hq, hkv, D, cache, li, 1)
        o = ops.decode_attention_fp8(q.view(B, 1, hq, D), cache.k[li], cache.v[li], cache.k_scale[li],
                                     cache.v_scale[li], seqlens_k=lens)
    else:
        o = ops.flash_attention(q.view(B, 1, hq, D), cache.k[li], cache.v[li], causal=False, seqlens_k=lens)
    h = K.gemv_fused(o.reshape(B, hq * D), attn.o_proj.weight, ws.sumsq, 0, res=h)
    gu = K.gemv_fused(h, mlp.gate_up_proj.weight, ws.sumsq, 0, g=ln2.weight, eps=ln2.eps)
    return K.gemv_fused(gu, mlp.down_proj.weight, ws.sumsq, 1, swiglu=True, res=h)


_DEVICE_SAMPLER = os.environ.get("GRT_DEVICE_SAMPLER", "1") != "0"
SAMPLER_MAX_EOS = 8  # kSampleMaxEos (csrc/include/grt_kernels.h)


@dataclass
class SamplerConfig:
    """What the device sampler at the end of a captured decode step does (``sample_logits``)."""
    max_new_tokens: int
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0          # 0: off
    top_p: float = 1.0      # 1.0: off
    seed: int = 0
    eos_ids: Tuple[int, ...] = ()
    pad_id: Optional[int] = None


SPEC_MAX_DRAFTS = 3  # kSpecMaxDrafts (csrc/include/grt_kernels.h): K + 1 <= 4 rows, the GEMV family's limit


@dataclass
class SpecConfig:
    """Prompt-lookup speculative decoding in the captured step: ``num_tokens`` = K drafts per step
    (1-3), ``max_ngram`` = N, the longest n-gram of the lookup. ``plan`` is a TEST HOOK, not an
    interface: an int64 device tensor that replaces the lookup, the drafts for token number n
    being ``plan[n : n + K]`` (-1 past its end). A random-init model never copies its prompt, so
    this is the one way to exercise acceptance deterministically."""
    num_tokens: int
    max_ngram: int = 2
    plan: Optional[torch.Tensor] = None


class GraphDecoder:
    """One-token decode step captured in a HIP graph (see module doc).

    Without a sampler the step returns logits and the caller picks the token: ``dec =
    GraphDecoder(model, B, max_len)``; ``logits = dec.prefill(ids)`` (eager, any prompt length);
    then ``logits = dec.step(next_ids)`` per token (graph replay).

    With ``sampler=SamplerConfig(...)`` the captured step ends in the device sampler, which also
    feeds the next step: ``dec.first_token(dec.prefill(ids))`` picks token 0 with the same op,
    eagerly, then ``dec.advance()`` per token is nothing but a graph replay. Tokens land in
    ``dec.out[:, n]``, ``dec.finished`` / ``dec.finish_step`` hold the EOS state.

    With ``spec=SpecConfig(K, N)`` (one sequence) the step is the VERIFY step of prompt-lookup
    speculative decoding: it runs T = K + 1 tokens, the last emitted one and K drafts, and with a
    sampler ends in the sampler's candidate mode and ``spec_advance`` (csrc/kernels/spec.hip),
    which accepts the agreeing drafts, emits 1 .. T tokens, moves every position on by that
    number and drafts for the next replay. ``n_replays`` / ``n_emitted`` count both. Without a
    sampler ``step_spec(ids, p)`` returns the logits [T, V] and the host does the rest.

    ``kv_cache_dtype="fp8"`` stores the cache as e4m3fn codes (see module doc); every mode above
    takes it.

    Needs a bf16 Llama on the GPU with head_dim 128 or 64 (the HIP RoPE epilogue / decode
    attention kernels)."""

    def __init__(self, model, B: int, max_len: int, sampler: Optional[SamplerConfig] = None,
                 spec: Optional[SpecConfig] = None, kv_cache_dtype=None):
        self.model = model
        self.spec = spec
        self.T = 1
        if spec is not None:
            if not 1 <= spec.num_tokens <= SPEC_MAX_DRAFTS:
                raise ValueError(f"SpecConfig.num_tokens must be in 1..{SPEC_MAX_DRAFTS}, got {spec.num_tokens}")
            if spec.max_ngram < 1:
                raise ValueError(f"SpecConfig.max_ngram must be >= 1, got {spec.max_ngram}")
            if B != 1:
                raise ValueError(f"speculative decoding takes one sequence, got a batch of {B}")
            self.T = spec.num_tokens + 1
        T = self.T
        self.n_replays = 0
        self.device = dev = next(model.parameters()).device
        kv = _kv_dtype(model, kv_cache_dtype)
        _check_fp8_decode(kv == "fp8", dev.type == "cuda", next(model.parameters()).dtype, model.config.head_dim)
        self.cache = KVCache(model.config, B, max_len, dev, kv)
        self.B = B
        self.cos, self.sin = model.rope(max_len, dev)
        self.ids = torch.zeros(B, T, dtype=torch.long, device=dev)
        self.pos_b = torch.zeros(B * T, dtype=torch.int32, device=dev)   # RoPE positions = cache slots
        self.lens = torch.zeros(B, dtype=torch.int32, device=dev)        # valid keys incl. new token
        self.graph = None
        self.logits = None
        # residual adds / norms inside the GEMVs when every projection is a plain bf16 Linear
        self.norm_ws = (_NormWorkspace(B, dev)
                        if dev.type == "cuda" and spec is None and _norm_fusable(model, B) else None)
        self.sampler = sampler
        if sampler is not None:
            if len(sampler.eos_ids) > SAMPLER_MAX_EOS:
                raise ValueError(f"the device sampler takes at most {SAMPLER_MAX_EOS} EOS ids, got {len(sampler.eos_ids)}")
            if sampler.max_new_tokens < 1:
                raise ValueError("SamplerConfig.max_new_tokens must be >= 1")
            self.finished = torch.zeros(B, dtype=torch.bool, device=dev)
            self.finish_step = torch.full((B,), -1, dtype=torch.long, device=dev)
            self.n_step = torch.zeros(1, dtype=torch.long, device=dev)    # column of `out` the next token takes
            self.counter = torch.zeros(1, dtype=torch.long, device=dev)   # noise counter: one per token
            self.out = torch.zeros(B, sampler.max_new_tokens, dtype=torch.long, device=dev)
            self.eos_t = (torch.tensor(sorted(sampler.eos_ids), dtype=torch.long, device=dev)
                          if sampler.eos_ids else None)
        if spec is not None:
            self._ar = torch.arange(T, dtype=torch.int32, device=dev)
            self.cand = torch.zeros(T, dtype=torch.long, device=dev)              # the sampler's candidates
            self.drafts = torch.full((T - 1,), -1, dtype=torch.long, device=dev)  # as drawn (-1: none)
            self.done = torch.zeros(1, dtype=torch.bool, device=dev)              # finished or full
            self.hist = None        # prompt + emitted tokens, allocated by prefill
            self.prompt_len = 0
            if spec.plan is not None and (spec.plan.dtype != torch.long or spec.plan.device != dev):
                raise ValueError("SpecConfig.plan must be an int64 tensor on the model's device")

    @property
    def n_emitted(self) -> int:
        """Tokens emitted so far (one host read)."""
        return int(self.n_step.item())

    def _spec_sample(self, logits: torch.Tensor) -> None:
        """Candidates of the T logits rows, then accept / emit / advance / draft on the device."""
        c, K = self.sampler, _native.kernels()
        if logits.dtype not in (torch.bfloat16, torch.float32):
            logits = logits.float()
        rows = logits.shape[0]  # 1 for the prefill logits: only cand[0] is read, no draft can match
        K.sample_logits(logits, do_sample=c.do_sample, temperature=c.temperature, top_k=c.top_k, top_p=c.top_p,
                        seed=c.seed, counter=self.counter, next_ids=self.cand[:rows], candidates=True)
        K.spec_advance(self.cand, self.drafts, self.ids.view(self.T), self.pos_b, self.lens, self.n_step, self.counter,
                       self.finished, self.finish_step, self.done, self.out.view(-1), self.hist, self.prompt_len,
                       c.max_new_tokens, self.spec.max_ngram, self.model.config.vocab_size, plan=self.spec.plan,
                       eos_ids=self.eos_t)

    def _sample(self, logits: torch.Tensor) -> None:
        """Pick one token per row with the device sampler and do the loop's bookkeeping: the token
        goes to ``ids`` (the next step's embedding input) and ``out[:, n_step]``; then both
        counters move on. All of it device work on the current stream (graph-capturable)."""
        c = self.sampler
        if logits.dtype not in (torch.bfloat16, torch.float32):
            logits = logits.float()
        _native.kernels().sample_logits(
            logits, do_sample=c.do_sample, temperature=c.temperature, top_k=c.top_k, top_p=c.top_p, seed=c.seed,
            counter=self.counter, finished=self.finished, finish_step=self.finish_step, step=self.n_step,
            next_ids=self.ids.view(self.B), out=self.out, eos_ids=self.eos_t, pad_id=c.pad_id,
            max_steps=c.max_new_tokens)
        self.counter.add_(1)
        self.n_step.add_(1)

    @torch.no_grad()
    def first_token(self, logits: torch.Tensor) -> None:
        """Token 0 from the prefill logits: the captured step's sampler call, run eagerly."""
        if self.spec is not None:
            self.drafts.fill_(-1)  # nothing was drafted for the prefill: exactly one token is emitted
            return self._spec_sample(logits[:1])
        self._sample(logits)

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor, attention_mask=None) -> torch.Tensor:
        """Eager prefill. With a padded batch (``attention_mask``, see ``forward_cached``) every
        row then decodes from its own length: the step's position and valid-length tensors differ
        per row, the captured step itself is the same."""
        if self.spec is not None:
            return self._spec_prefill(input_ids, attention_mask)
        logits = forward_cached(self.model, input_ids, self.cache, attention_mask)
        n = self.cache.len
        if self.cache.lens is None:
            self.pos_b.fill_(n)
            self.lens.fill_(n + 1)
        else:
            self.pos_b.copy_(self.cache.lens)
            self.lens.copy_(self.cache.lens + 1)
            self.cache.lens = self.pos_b  # the replays advance it
        return logits

    def _spec_prefill(self, input_ids: torch.Tensor, attention_mask=None) -> torch.Tensor:
        """Prefill of the one row (a padded row's tokens are compacted as in ``forward_cached``;
        from then on nothing differs). The positions are left one short of the first verify step's:
        ``first_token`` emits exactly one token and ``spec_advance`` moves them on by it."""
        rows = _mask_rows(attention_mask, 1, input_ids.shape[1])
        prompt = _row_prompt(input_ids, rows)
        logits = forward_cached(self.model, input_ids, self.cache, rows)
        n = prompt.shape[0]
        self.cache.len, self.cache.lens = n, None
        self.prompt_len = n
        new = self.sampler.max_new_tokens if self.sampler is not None else 0
        self.hist = torch.zeros(n + new, dtype=torch.long, device=self.device)
        self.hist[:n] = prompt
        self.pos_b.copy_(self._ar + (n - 1))
        self.lens.fill_(n - 1 + self.T)
        return logits

    @torch.no_grad()
    def _step_body(self):
        """Embedding, layers, logits [B * T, V], tail."""
        m, B, T = self.model, self.B, self.T
        h = m.model.embed_tokens(self.ids).view(B * T, -1)
        if self.norm_ws is not None:
            for li, layer in enumerate(m.model.layers):
                h = _fused_norm_layer_step(layer, h, li == 0, self.norm_ws, B, self.cos, self.sin,
                                           self.cache, li, self.pos_b, self.lens)
            fn = m.model.norm
            logits = _native.kernels().gemv_fused(h, m.lm_head.weight, self.norm_ws.sumsq, 1, g=fn.weight,
                                                  eps=fn.eps)
        else:
            logits = m.lm_head(_layers(m, h, lambda li, attn, qkv: _device_attention(
                attn, qkv, B, T, self.cos, self.sin, self.cache, li, self.pos_b, self.lens)))
        return self._step_tail(logits)

    def _step_tail(self, logits):
        """End of the step: the sampler reads the LM head's bf16 logits as they are; without one
        the caller gets an fp32 copy. Then the positions move on by one token; those of a verify
        step are moved by ``spec_advance``, by the number of tokens emitted, or set by ``step_spec``."""
        if self.sampler is None:
            logits = logits.float()
        elif self.spec is not None:
            self._spec_sample(logits)
        else:
            self._sample(logits)
        if self.spec is None:
            self.pos_b.add_(1)
            self.lens.add_(1)
        return logits

    def _capture(self):
        # warm up on a side stream (allocator pools, library handles), then capture one step;
        # the warm-up step's cache writes land at the current position and are rewritten by the
        # first replay, and the position tensors are restored afterwards
        state = [self.pos_b, self.lens]
        if self.sampler is not None:  # the sampler's epilogue writes these; column n_step of `out`
            # is written again, with the same token, by the first replay
            state += [self.ids, self.finished, self.finish_step, self.n_step, self.counter]
            if self.spec is not None:  # out / hist past n_step are rewritten alike by the first replay
                state += [self.drafts, self.done, self.cand]
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self._step_body()
        torch.cuda.current_stream(self.device).wait_stream(s)
        for t, v in zip(state, saved):
            t.copy_(v)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._step_body()
        for t, v in zip(state, saved):
            t.copy_(v)

    @torch.no_grad()
    def advance(self) -> None:
        """One more token on the device: a graph replay and nothing else (needs a sampler; the
        previous token is already in ``ids``)."""
        if self.sampler is None:
            raise RuntimeError("GraphDecoder.advance() needs a SamplerConfig; use step(next_ids)")
        if self.spec is not None:
            # the positions live on the device and a finished or full row is inert: a replay past the
            # end writes cache slots below prompt + max_new_tokens + K only (generate() sizes the
            # cache so), and rope_append skips any position outside the cache
            return self._replay()
        if self.cache.len >= self.cache.max_len:
            raise RuntimeError("KV cache full")
        self._replay()
        self.cache.len += 1

    def _replay(self) -> None:
        """One replay of the captured step, captured at the first one."""
        if self.graph is None:
            self._capture()
        self.graph.replay()
        self.n_replays += 1

    @torch.no_grad()
    def step_spec(self, ids: torch.Tensor, p: int) -> torch.Tensor:
        """Host-loop verify step: ``ids`` [T] = the last emitted token and K drafts at positions
        p ... p + K. Returns the logits [T, V] (the graph's buffer)."""
        if self.spec is None or self.sampler is not None:
            raise RuntimeError("GraphDecoder.step_spec() is the sampler-less step of a SpecConfig decoder")
        if p + self.T > self.cache.max_len:
            raise RuntimeError("KV cache full")
        self.ids.copy_(ids.view(1, self.T))
        self.pos_b.copy_(self._ar + p)
        self.lens.fill_(p + self.T)
        self._replay()
        return self.logits

    @torch.no_grad()
    def step(self, next_ids: torch.Tensor) -> torch.Tensor:
        if self.sampler is not None:
            raise RuntimeError("GraphDecoder.step() returns logits; with a SamplerConfig use advance()")
        if self.spec is not None:
            raise RuntimeError("GraphDecoder.step() takes one token; with a SpecConfig use step_spec(ids, p)")
        if self.cache.len >= self.cache.max_len:
            raise RuntimeError("KV cache full")
        self.ids.copy_(next_ids.view(self.B, 1))
        self._replay()
        self.cache.len += 1
        return self.logits


def _graph_ok(model, input_ids) -> bool:
    p = next(model.parameters())
    cfg = model.config
    return (input_ids.is_cuda and p.dtype == torch.bfloat16 and cfg.head_dim in (64, 128)
            and _native.kernels_available())


def _device_loop_ok(graph: bool, generator, n_eos: int, max_new_tokens: int) -> bool:
    return (graph and generator is None and n_eos <= SAMPLER_MAX_EOS and max_new_tokens >= 1
            and _native.kernels_available())


last_spec_stats = {"n_replays": 0, "n_emitted": 0}  # of the latest speculative generate()


def _spec_generate(model, input_ids, rows, P: int, sampler: SamplerConfig, spec: SpecConfig, graph: bool,
                   on_device: bool, sync_every: int, kv=None) -> torch.Tensor:
    """The new tokens [n] of one sequence by prompt-lookup speculative decoding (see ``generate``)."""
    K, new = spec.num_tokens, sampler.max_new_tokens
    dev = input_ids.device
    max_len = P + new + K
    if on_device:
        dec = GraphDecoder(model, 1, max_len, sampler=sampler, spec=spec, kv_cache_dtype=kv)
        dec.first_token(dec.prefill(input_ids, rows))
        left = new - 1  # every replay of a live row emits at least one token
        while left > 0:
            chunk = min(sync_every, left)
            for _i in range(chunk):
                dec.advance()
            left -= chunk
            if left > 0 and bool(dec.done):  # the one host read per chunk: finished or full
                break
        n = dec.n_emitted
        last_spec_stats.update(n_replays=dec.n_replays, n_emitted=n)
        return dec.out[0, :n]
    prompt = _row_prompt(input_ids, rows)
    if graph:
        dec = GraphDecoder(model, 1, max_len, spec=spec, kv_cache_dtype=kv)
        first = dec.prefill(input_ids, rows)

        def step(ids, p):
            return dec.step_spec(torch.tensor(ids, device=dev), p)
    else:
        cache = KVCache(model.config, 1, max_len, dev, _kv_dtype(model, kv))
        first = forward_cached(model, input_ids, cache, rows)
        cache.lens = None  # one row: nothing is ragged once its tokens sit at 0 ... P - 1

        def step(ids, p):
            cache.len = p  # the slots of rejected drafts are rewritten
            return forward_cached(model, torch.tensor([ids], device=dev), cache, all_logits=True)[0]

    def pick(logits, n):  # the sampler's host implementation, row t at token number n + t
        if not sampler.do_sample:
            return logits.argmax(-1).tolist()
        return [int(_ref.sample_tokens(logits[t:t + 1], seed=sampler.seed, counter=n + t, temperature=sampler.temperature,
                                       top_k=sampler.top_k, top_p=sampler.top_p)) for t in range(logits.shape[0])]

    V = model.config.vocab_size
    plan = spec.plan.tolist() if spec.plan is not None else None
    hist = prompt.tolist()
    out, fin, _ = _ref.spec_accept([-1] * K, pick(first[:1], 0), 0, new, sampler.eos_ids)
    hist += out
    replays = 0
    while not fin and len(out) < new:
        n = len(out)
        if plan is not None:
            drafts = (plan[n:n + K] + [-1] * K)[:K]
        else:
            drafts = _ref.prompt_lookup_draft(hist, len(hist), K, spec.max_ngram)
        ids = [hist[-1]] + [d if 0 <= d < V else 0 for d in drafts]
        logits = step(ids, P + n - 1)
        emitted, fin, _ = _ref.spec_accept(drafts, pick(logits, n), n, new, sampler.eos_ids)
        out += emitted
        hist += emitted
        replays += 1
    last_spec_stats.update(n_replays=replays, n_emitted=len(out))
    return torch.tensor(out, dtype=torch.long, device=dev)


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int = 32,
             eos_token_id: Optional[Union[int, List[int]]] = None, do_sample: bool = False, temperature: float = 1.0,
             top_p: Optional[float] = None, attention_mask=None, pad_token_id=None, generator=None,
             use_graph: Optional[bool] = None, sync_every: int = 16, top_k: Optional[int] = None,
             seed: Optional[int] = None, device_loop: Optional[bool] = None,
             prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: int = 2, _spec_plan=None,
             kv_cache_dtype: Optional[str] = None, **_):
    """Returns [B, prompt + generated] token ids (HF ``generate`` output convention).

    ``attention_mask`` [B, S] (bool / integer, HF semantics) batches prompts of unequal length: row
    b's prompt is its masked tokens (one contiguous run; padding left, right or on both sides) at
    positions 0 ... len_b - 1, its t-th new token sits at position len_b + t and attends to that
    row's prompt and earlier new tokens only, and the ids in the pad columns influence nothing. A
    greedy row gives the tokens it gives alone. The result is ``input_ids`` as given (pads
    included) followed by the generated columns. ``None`` or all ones: no padding. A hole, an
    all-zero row or another shape raises ``ValueError``. Every decode path takes it (graph with
    either loop, eager): the per-row position and valid-length tensors of the step differ per row.

    A bf16 model on the GPU with head_dim 128 or 64 (``llama3.2-1b``) decodes through the HIP-graph
    decoder by default (fused RoPE epilogue of the qkv GEMV, split-K decode attention at either
    width). ``use_graph=False`` gives the eager step; ``GRT_DECODE_ATTN=0`` sends the one-token
    attention to the flash forward kernel with ``seqlens_k`` and ``GRT_GEMV_NORM=0`` keeps the
    norms and ``rope_append`` outside the GEMVs.

    Sampling (``do_sample=True``): ``temperature``, then ``top_k`` (None / 0: off; ties at the
    k-th value are all kept), then ``top_p`` over the renormalised survivors, as HF chains them.
    Without a ``generator`` the draw is a Gumbel-max over counter-based noise of (``seed``, token
    number, row, vocabulary index): the same ``seed`` and the same logits give the same tokens on
    the GPU and on the CPU. ``seed=None`` draws one from torch's default generator, so
    ``torch.manual_seed`` governs it. With a ``generator`` the draw is ``torch.multinomial``'s.

    On the graph path with no ``generator`` and at most 8 EOS ids, the token is picked inside the
    captured step by the device sampler (``device_loop``, default on; ``GRT_DEVICE_SAMPLER=0`` or
    ``device_loop=False`` restore the host loop): the loop is graph replays and one host read of
    ``finished.all()`` every ``sync_every`` tokens.

    ``prompt_lookup_num_tokens`` = K in 1..3 (None / 0: off, the default) with
    ``max_matching_ngram_size`` = N (HF's names; N defaults to 2) turns on prompt-lookup
    speculative decoding for ONE sequence: every step drafts K tokens by looking the last n <= N
    tokens up in the prompt and the tokens so far (``_ref.prompt_lookup_draft``), runs the last
    token and the drafts as one T = K + 1 row verify step, and keeps the drafts that equal the
    token the sampler draws at their token number, plus one (``_ref.spec_accept``). Because the
    sampler's noise depends on the token number alone, that rule is exact for greedy and for
    ``do_sample=True``: the output is what the same call gives without drafts, up to near-ties in
    the logits, which the 1-row and the T-row kernels may round differently. The cache holds
    prompt + ``max_new_tokens`` + K positions. Every decode path takes it: on the graph path with
    the device loop the draft, the candidates and the accept step run inside the captured step
    (csrc/kernels/spec.hip) and the host reads one "finished or full" flag every ``sync_every``
    replays; the graph host loop and the eager path do them on the host. ``ValueError``: K outside
    1..3, N < 1, more than one sequence, a ``generator``, or prompt + ``max_new_tokens`` + K past
    ``max_position_embeddings``. ``_spec_plan`` is a private test hook (``SpecConfig.plan``).
    ``last_spec_stats`` holds the verify steps and tokens of the latest such call.

    ``kv_cache_dtype``: ``None`` / ``"auto"`` keeps the cache in the model's dtype; ``"fp8"`` /
    ``"fp8_e4m3"`` stores it as e4m3fn codes with one fp32 scale per (token, kv head), (D + 4) / 2D of
    the bf16 bytes (see the module doc: the prefill logits are those of the bf16 cache, decode
    tokens attend to the quantised cache, the captured one-token step has one more launch per
    layer, a chunk of more than 4 tokens on a non-empty cache takes a dequantising slow path).
    Every mode above takes it. ``ValueError``: another value, or ``GRT_DECODE_ATTN=0`` with the fp8
    cache on the GPU."""
    was = model.training
    model.eval()
    try:
        B, S = input_ids.shape
        kv = "fp8" if _kv_dtype(model, kv_cache_dtype) == "fp8" else None
        _check_fp8_decode(kv == "fp8", input_ids.is_cuda, next(model.parameters()).dtype, model.config.head_dim)
        rows = _mask_rows(attention_mask, B, S)
        P = S if rows is None else max(rows.lens)  # the longest prompt: the cache holds P + max_new_tokens
        eos = set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))
        graph = use_graph if use_graph is not None else _graph_ok(model, input_ids)
        temperature = max(temperature, 1e-5)
        top_k = int(top_k) if top_k else 0
        top_p = 1.0 if top_p is None else float(top_p)
        if top_k < 0 or not 0.0 < top_p <= 1.0:
            raise ValueError(f"generate: top_k must be >= 0 and top_p in (0, 1], got top_k={top_k}, top_p={top_p}")
        if do_sample and generator is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # torch's default generator: torch.manual_seed governs
        seed = int(seed or 0)
        can = _device_loop_ok(graph, generator, len(eos), max_new_tokens)
        if device_loop and not can:
            raise ValueError("generate: device_loop=True needs the graph path (bf16 model on the GPU, native kernels), "
                             f"no generator, at most {SAMPLER_MAX_EOS} EOS ids and max_new_tokens >= 1")
        K = int(prompt_lookup_num_tokens or 0)
        if K:
            N = int(max_matching_ngram_size)
            limit = model.config.max_position_embeddings
            if not 1 <= K <= SPEC_MAX_DRAFTS:
                raise ValueError(f"generate: prompt_lookup_num_tokens must be in 1..{SPEC_MAX_DRAFTS} (the verify step "
                                 f"runs K + 1 <= {SPEC_MAX_DRAFTS + 1} rows, the limit of the GEMV kernels), got {K}")
            if N < 1:
                raise ValueError(f"generate: max_matching_ngram_size must be >= 1, got {N}")
            if B != 1:
                raise ValueError(f"generate: prompt lookup decoding takes a batch of 1, got {B} sequences")
            if generator is not None:
                raise ValueError("generate: prompt lookup decoding needs the counter-based noise (seed=...), not a "
                                 "torch generator: a draft is accepted iff it is the token drawn at its token number")
            if P + max_new_tokens + K > limit:
                raise ValueError(f"generate: prompt ({P}) + max_new_tokens ({max_new_tokens}) + "
                                 f"prompt_lookup_num_tokens ({K}) exceeds max_position_embeddings ({limit}), the "
                                 "extent of the RoPE table")
        sampler = SamplerConfig(max_new_tokens=max_new_tokens, do_sample=do_sample, temperature=temperature, top_k=top_k,
                                top_p=top_p, seed=seed, eos_ids=tuple(sorted(eos)), pad_id=pad_token_id)
        on_device = can and (device_loop if device_loop is not None else _DEVICE_SAMPLER)
        if K and max_new_tokens >= 1:
            new = _spec_generate(model, input_ids, rows, P, sampler, SpecConfig(K, N, _spec_plan), graph, on_device,
                                 sync_every, kv)[None]
        elif on_device:
            new = _device_loop(model, input_ids, rows, P, sampler, sync_every, kv)
        else:
            new = _host_loop(model, input_ids, rows, P, sampler, graph, generator, sync_every, kv)
        return torch.cat([input_ids, new], 1)
    finally:
        if was:
            model.train()


def _device_loop(model, input_ids, rows, P: int, sampler: SamplerConfig, sync_every: int, kv=None) -> torch.Tensor:
    """The new tokens [B, n] with the token picked inside the captured step."""
    new, eos = sampler.max_new_tokens, sampler.eos_ids
    dec = GraphDecoder(model, input_ids.shape[0], P + new, sampler=sampler, kv_cache_dtype=kv)
    dec.first_token(dec.prefill(input_ids, rows))
    done = 1
    while done < new:
        # replays up to the next multiple of sync_every tokens, then one host read
        for _i in range(min(sync_every - done % sync_every, new - done)):
            dec.advance()
            done += 1
        if eos and done % sync_every == 0 and bool(dec.finished.all()):
            break
    if eos:  # HF stops right after the token that finished the last row
        last = dec.finish_step.tolist()
        if min(last) >= 0:
            done = max(last) + 1
    return dec.out[:, :done]


def _multinomial_pick(logits, temperature: float, top_k: int, top_p: float, generator) -> torch.Tensor:
    """A ``torch.multinomial`` draw per row after temperature, top-k and top-p, as HF chains them."""
    probs = torch.softmax(logits / temperature, -1)
    if 0 < top_k < probs.shape[-1]:
        kth = probs.topk(top_k, -1).values[..., -1:]
        probs = torch.where(probs < kth, torch.zeros_like(probs), probs)
        probs = probs / probs.sum(-1, keepdim=True)
    if top_p < 1.0:
        sp, si = probs.sort(-1, descending=True)
        keep = sp.cumsum(-1) - sp <= top_p
        sp = sp * keep
        probs = torch.zeros_like(probs).scatter(-1, si, sp)
    return torch.multinomial(probs / probs.sum(-1, keepdim=True), 1, generator=generator).squeeze(-1)


def _host_loop(model, input_ids, rows, P: int, c: SamplerConfig, graph: bool, generator, sync_every: int, kv=None):
    """The new tokens [B, n], picked on the host from the logits of the graph's or the eager step."""
    B, new = input_ids.shape[0], c.max_new_tokens
    if graph:
        dec = GraphDecoder(model, B, P + new, kv_cache_dtype=kv)
        logits = dec.prefill(input_ids, rows)
        forward = dec.step
    else:
        cache = KVCache(model.config, B, P + new, input_ids.device, _kv_dtype(model, kv))
        logits = forward_cached(model, input_ids, cache, rows)

        def forward(nxt):
            return forward_cached(model, nxt[:, None], cache)
    eos_t = torch.tensor(list(c.eos_ids), device=input_ids.device) if c.eos_ids else None
    out = []
    finished = torch.zeros(B, dtype=torch.bool, device=input_ids.device)
    all_done = []  # device flags: every row finished after token t
    for t in range(new):
        if c.do_sample and generator is None:
            # the device sampler's host implementation: token t draws the noise of counter t
            nxt = _ref.sample_tokens(logits, seed=c.seed, counter=t, temperature=c.temperature, top_k=c.top_k,
                                     top_p=c.top_p)
        elif c.do_sample:
            nxt = _multinomial_pick(logits, c.temperature, c.top_k, c.top_p, generator)
        else:
            nxt = logits.argmax(-1)
        if c.pad_id is not None:
            nxt = torch.where(finished, torch.full_like(nxt, c.pad_id), nxt)
        out.append(nxt[:, None])
        if eos_t is not None:
            finished |= torch.isin(nxt, eos_t)
            all_done.append(finished.all())
            if (t + 1) % sync_every == 0 and bool(finished.all()):
                break
        if t + 1 < new:
            logits = forward(nxt)
    if all_done:  # HF stops right after the token that finished the last row
        flags = torch.stack(all_done)
        if bool(flags.any()):
            out = out[:int(flags.nonzero()[0, 0]) + 1]
    return torch.cat([input_ids[:, :0], *out], 1)  # [B, 0] when there is no new token
