"""Hot-path ops: gfx950 HIP kernels on GPU tensors, PyTorch references on CPU tensors."""
from .fused import (add_rms_norm, cross_entropy, decode_attention_fp8, decode_attention_multi, dropout,
                    flash_attention, gelu, layer_norm, lm_head_cross_entropy, nf4_dequantize, nf4_gemv, nf4_quantize,
                    rms_norm, rope_attention, swiglu, Varlen)
from .optim import AdamW8bit, FusedAdamW, GradClipState, clip_grad_norm_, make_optimizer
from ._ref import rope_tables

__all__ = [
    "add_rms_norm", "cross_entropy", "decode_attention_fp8", "decode_attention_multi", "dropout", "flash_attention",
    "gelu", "layer_norm", "lm_head_cross_entropy", "nf4_dequantize", "nf4_gemv", "nf4_quantize", "rms_norm",
    "rope_attention", "swiglu", "Varlen",
    "AdamW8bit", "FusedAdamW", "GradClipState", "clip_grad_norm_", "make_optimizer", "rope_tables",
]
