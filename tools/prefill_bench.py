#!/usr/bin/env python3
"""Chunked prefill of a 4-bit (QLoRA) model without the dequant cache: the tile MFMA GEMM from the
NF4 codes (csrc/kernels/gemm_nf4_tile.hip) against the parent path, which dequantises every
projection for every chunk. Llama-3.1-8B architecture, random init, LoRA r on all 7 targets, batch 1,
a prompt of ``--prompt`` tokens in chunks of ``--chunks`` tokens. The two arms alternate ``--rounds``
times in this one process; the parent path is selected by ``quant.NF4_TILE_MAX_ROWS = 16``. One JSON
line per (round, chunk size, arm): seconds of the whole prefill, host clock around a synchronise.

    python tools/prefill_bench.py [llama3.1-8b] [--prompt 2048] [--chunks 32,64,128,256] [--r 64]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd.models import build_llama  # noqa: E402
from gke_ray_train_amd.models.generation import KVCache, _prefill  # noqa: E402
from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quant, quantize_model_  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="llama3.1-8b")
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--chunks", default="32,64,128,256")
    ap.add_argument("--r", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=0, help="build only this many layers (0: the model's own)")
    a = ap.parse_args()
    over = dict(num_hidden_layers=a.layers) if a.layers else {}
    net = build_llama(a.model, device="cuda", dtype=torch.bfloat16, seed=0, **over)
    quantize_model_(net, BitsAndBytesConfig())
    quant.set_dequant_cache(net, "0")
    pm = get_peft_model(net, LoraConfig(r=a.r, lora_alpha=16))
    for lw in pm.lora_modules.values():
        for p in lw.lora_B.values():
            p.data.normal_(0, 0.02)
    pm.eval()
    model = pm.base_model
    ids = torch.randint(0, net.config.vocab_size, (1, a.prompt), device="cuda")

    def run(c):
        cache = KVCache(model.config, 1, a.prompt, ids.device, torch.bfloat16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logits = _prefill(model, ids, cache, None, c)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, logits

    with torch.no_grad():
        for rnd in range(a.rounds):
            for c in [int(v) for v in a.chunks.split(",")]:
                ref = None
                for arm, limit in (("dequantise", 16), ("codes", quant.NF4_TILE_KERNEL_ROWS)):
                    quant.NF4_TILE_MAX_ROWS = limit
                    run(c)  # warm-up of this arm's shapes
                    dt, logits = run(c)
                    ref = logits if ref is None else ref
                    print(json.dumps({"model": a.model, "layers": model.config.num_hidden_layers, "lora_r": a.r,
                                      "prompt": a.prompt, "chunk": c, "arm": arm, "round": rnd,
                                      "prefill_s": round(dt, 4), "tokens_per_s": round(a.prompt / dt, 1),
                                      "argmax_as_dequantise": bool((logits.argmax(-1) == ref.argmax(-1)).all()),
                                      "max_logit_diff": round((logits - ref).abs().max().item(), 4)}), flush=True)


if __name__ == "__main__":
    main()
