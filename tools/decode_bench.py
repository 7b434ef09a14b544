"""Decode throughput on MI355X: eager cached decode vs the HIP-graph decoder (models/generation.py).
Llama-3.1-8B architecture, random init, bf16, batch 1, prompt 512, 128 new tokens (the
reference's inference comparison generates up to MAX_NEW_GENERATION_TOKENS_INFERENCE = 300
tokens per sample, ray-jobs/fine_tune_config.json:35). One JSON line per mode.

``DECODE_QUANT=nf4`` (optionally ``DECODE_LORA=<r>``: LoRA on all 7 targets, non-zero lora_B) times
HIP-graph decode from a 4-bit base instead: the NF4 GEMV (csrc/kernels/gemv_nf4.hip) against the dequantising path it replaces, with the dequant cache
on and off, the arms alternating ``DECODE_ROUNDS`` (2) times in this one process. ``DECODE_CACHE=0|1``
keeps one cache mode (70B: 0); ``DECODE_B`` may be a comma list here.

``DECODE_SAMPLE=greedy|top_p`` and / or ``DECODE_DEVICE_LOOP=0|1`` times the HIP-graph decoder with the
token picked on the device inside the captured step against the host loop (``sampler_main``).

``DECODE_SPEC=K`` (a comma list of 1-3) times prompt-lookup speculative decoding (``generate(...,
prompt_lookup_num_tokens=K)``, device loop) against the plain device loop (``spec_main``).

``DECODE_ATTN=1`` times the multi-token decode attention kernel alone against T launches of the
one-token kernel (``attn_main``).

``DECODE_KV=fp8`` times the fp8 KV cache (``generate(..., kv_cache_dtype="fp8")``) against the bf16
cache, device loop, ``DECODE_B`` sequences with a prompt of ``DECODE_PROMPT`` (512) tokens
(``kv_main``); with ``DECODE_ATTN=1`` it times the decode attention kernel alone over an fp8 and a
bf16 cache instead (``kv_attn_main``)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd.models import build_llama  # noqa: E402

QUANT = os.environ.get("DECODE_QUANT", "")
model = sys.argv[1] if len(sys.argv) > 1 else "llama3.1-8b"
B_ENV = os.environ.get("DECODE_B", "1")  # sequences decoded together (batch of requests)


def nf4_main():
    from gke_ray_train_amd.peft import BitsAndBytesConfig, LoraConfig, get_peft_model, quantize_model_
    from gke_ray_train_amd.peft import quant
    if QUANT != "nf4":
        sys.exit("DECODE_QUANT: only nf4")
    r = int(os.environ.get("DECODE_LORA", "0"))
    new = int(os.environ.get("DECODE_NEW", "128"))
    net = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0)
    cfg = net.config
    quantize_model_(net, BitsAndBytesConfig())
    net = get_peft_model(net, LoraConfig(r=r, lora_alpha=16)) if r else net
    if r:
        for lw in net.lora_modules.values():
            for p in lw.lora_B.values():
                p.data.normal_(0, 0.02)
    net.eval()
    base = net.base_model if r else net
    caches = [c for c in ("1", "0") if os.environ.get("DECODE_CACHE", c) == c]
    for B in [int(b) for b in B_ENV.split(",")]:  # here DECODE_B may be a list: one model build for all
        ids = torch.randint(0, cfg.vocab_size, (B, 512), device="cuda")
        nf4_arms(net, base, quant, ids, B, r, new, caches)


def nf4_arms(net, base, quant, ids, B, r, new, caches):
    for rnd in range(int(os.environ.get("DECODE_ROUNDS", "2"))):
        for cache in caches:
            for kern in (False, True):
                quant.set_dequant_cache(base, cache)
                quant._NF4_GEMV = kern
                net.generate(ids, max_new_tokens=8, use_graph=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.generate(ids, max_new_tokens=2, use_graph=True)  # prefill, capture and one replay
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                out = net.generate(ids, max_new_tokens=new, use_graph=True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                step = (dt - (t1 - t0)) / (new - 2)  # seconds per replayed step
                print(json.dumps({"model": model, "quant": "nf4", "lora_r": r, "dequant_cache": cache == "1",
                                  "nf4_gemv": kern, "batch": B, "round": rnd, "new_tokens": out.shape[1] - 512,
                                  "seconds": round(dt, 3),
                                  "tokens_per_s": round(B * (out.shape[1] - 512) / dt, 1),
                                  "decode_step_ms": round(step * 1e3, 3),
                                  "decode_tokens_per_s": round(B / step, 1)}), flush=True)
        torch.cuda.empty_cache()


def sampler_main():
    """``DECODE_SAMPLE=greedy|top_p`` and / or ``DECODE_DEVICE_LOOP=0|1``: HIP-graph decode with the
    token picked by the device sampler inside the captured step (device loop) against the host loop
    on the graph's logits. ``top_p``: do_sample, top_p 0.9, seed 0. Unset ``DECODE_DEVICE_LOOP`` runs
    both loops, alternating, ``DECODE_ROUNDS`` (3) times in this one process; ``DECODE_NEW`` tokens."""
    sample = os.environ.get("DECODE_SAMPLE", "greedy")
    if sample not in ("greedy", "top_p"):
        sys.exit("DECODE_SAMPLE: greedy or top_p")
    loops = [bool(int(v)) for v in os.environ.get("DECODE_DEVICE_LOOP", "0,1").split(",")]
    new = int(os.environ.get("DECODE_NEW", "128"))
    B = int(B_ENV)
    net = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0).eval()
    ids = torch.randint(0, net.config.vocab_size, (B, 512), device="cuda")
    kw = dict(do_sample=True, top_p=0.9, seed=0) if sample == "top_p" else {}
    for rnd in range(int(os.environ.get("DECODE_ROUNDS", "3"))):
        for loop in loops:
            net.generate(ids, max_new_tokens=8, use_graph=True, device_loop=loop, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.generate(ids, max_new_tokens=2, use_graph=True, device_loop=loop, **kw)  # prefill, capture, one replay
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = net.generate(ids, max_new_tokens=new, use_graph=True, device_loop=loop, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            step = (dt - (t1 - t0)) / (new - 2)  # seconds per token after the first two
            print(json.dumps({"model": model, "sample": sample, "device_loop": loop, "batch": B, "round": rnd,
                              "new_tokens": out.shape[1] - 512, "seconds": round(dt, 3),
                              "tokens_per_s": round(B * (out.shape[1] - 512) / dt, 1),
                              "ms_per_token": round(step * 1e3, 3)}), flush=True)


def spec_main():
    """``DECODE_SPEC=K[,K...]``: greedy, batch 1, prompt 512, ``DECODE_NEW`` (128) tokens. The drafts
    come from the test hook ``_spec_plan`` so that the acceptance is forced: the run's own tokens
    (100 %: every verify step emits K + 1 tokens), the same with every second token wrong (50 %)
    and with every token wrong (0 %: every step emits 1 token, so its time is the verify step's).
    The plain device loop and the speculative arms alternate ``DECODE_ROUNDS`` (2) times in this one
    process. ``ms_per_step`` is per graph replay; the replays include those past the last token up
    to the next host read (``sync_every`` 16), which emit nothing and cost a step each."""
    from gke_ray_train_amd.models import generation as G
    ks = [int(k) for k in os.environ["DECODE_SPEC"].split(",")]
    new = int(os.environ.get("DECODE_NEW", "128"))
    net = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0).eval()
    V = net.config.vocab_size
    ids = torch.randint(0, V, (1, 512), device="cuda")
    plain = net.generate(ids, max_new_tokens=new, use_graph=True)[0, 512:]
    arms = [("plain", 0, None, plain)]
    for K in ks:
        # A random-init model's logits are nearly flat, so the verify step (norms outside the GEMVs,
        # K + 1 rows) soon picks other tokens than the plain step: the plan that is accepted in full
        # is the speculative run's own output, found by feeding it back until it reproduces itself.
        plan = plain
        for _ in range(4):
            out = net.generate(ids, max_new_tokens=new, use_graph=True, prompt_lookup_num_tokens=K, _spec_plan=plan)
            if torch.equal(out[0, 512:], plan):
                break
            plan = out[0, 512:].clone()
        wrong = (plan + 1) % V
        half = torch.where(torch.arange(new, device="cuda") % 2 == 1, wrong, plan)
        arms += [(f"spec_{pct}", K, p, plan) for pct, p in (("100", plan), ("50", half), ("0", wrong))]
    for rnd in range(int(os.environ.get("DECODE_ROUNDS", "2"))):
        for name, K, plan, ref in arms:
            kw = dict(prompt_lookup_num_tokens=K, _spec_plan=plan) if K else {}
            net.generate(ids, max_new_tokens=8, use_graph=True, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.generate(ids, max_new_tokens=2, use_graph=True, **kw)  # prefill, capture, one replay
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = net.generate(ids, max_new_tokens=new, use_graph=True, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            n = out.shape[1] - 512
            replays = G.last_spec_stats["n_replays"] if K else n - 1
            same = int((out[0, 512:] == ref[:n]).sum())  # whatever the drafts, the tokens stay the same
            print(json.dumps({"model": model, "arm": name, "K": K, "round": rnd, "new_tokens": n, "replays": replays,
                              "tokens_as_without_drafts": same, "seconds": round(dt, 3),
                              "tokens_per_s": round(n / dt, 1),
                              "ms_per_step": round((dt - (t1 - t0)) / max(replays - 1, 1) * 1e3, 3),
                              "decode_tokens_per_s": round((n - 2) / (dt - (t1 - t0)), 1)}), flush=True)


def attn_main():
    """``DECODE_ATTN=1``: ``attn_decode_multi`` at T = 2, 3, 4 against T launches of ``attn_decode``
    (what verifying token by token costs), batch 1, 32 query / 8 kv heads, head_dim 128 and 64, a
    cache of 640 slots with 600 valid keys. Back-to-back launches timed with events, the two arms
    alternating ``DECODE_ROUNDS`` (3) times."""
    from gke_ray_train_amd import _native
    C = _native.kernels()
    iters = 300

    def timed(fn):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3

    for D in (128, 64):
        multi = C.attn_decode_multi if D == 128 else C.attn_decode_multi_d64
        one = C.attn_decode if D == 128 else C.attn_decode_d64
        k = torch.randn(1, 640, 8, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(1, 640, 8, D, device="cuda", dtype=torch.bfloat16)
        sl = torch.tensor([600], device="cuda", dtype=torch.int32)
        for T in (2, 3, 4):
            q = torch.randn(1, T, 32, D, device="cuda", dtype=torch.bfloat16)
            qs = [q[:, t:t + 1] for t in range(T)]
            for rnd in range(int(os.environ.get("DECODE_ROUNDS", "3"))):
                us_m = timed(lambda: multi(q, k, v, sl, D ** -0.5))
                us_1 = timed(lambda: [one(x, k, v, sl, D ** -0.5) for x in qs])
                print(json.dumps({"kernel": "attn_decode_multi", "head_dim": D, "T": T, "round": rnd,
                                  "multi_us": round(us_m, 2), "T_single_launches_us": round(us_1, 2)}), flush=True)


def kv_main():
    """``DECODE_KV=fp8``: greedy, ``DECODE_B`` sequences, prompt ``DECODE_PROMPT`` (512), ``DECODE_NEW``
    (128) tokens, HIP-graph decoder with the device loop; the bf16-cache and the fp8-cache arm
    alternate ``DECODE_ROUNDS`` (3) times in this one process. The replays are timed on their own
    with events (prefill, first token and the capturing replay come before the first event), so
    ``ms_per_step`` is the captured step and nothing else. ``cache_bytes`` is ``KVCache.nbytes()``."""
    from gke_ray_train_amd.models import generation as G
    if os.environ["DECODE_KV"] != "fp8":
        sys.exit("DECODE_KV: only fp8")
    new = int(os.environ.get("DECODE_NEW", "128"))
    P = int(os.environ.get("DECODE_PROMPT", "512"))
    B = int(B_ENV)
    net = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0).eval()
    ids = torch.randint(0, net.config.vocab_size, (B, P), device="cuda")
    for rnd in range(int(os.environ.get("DECODE_ROUNDS", "3"))):
        for kv in (None, "fp8"):
            dec = G.GraphDecoder(net, B, P + new, sampler=G.SamplerConfig(max_new_tokens=new), kv_cache_dtype=kv)
            dec.first_token(dec.prefill(ids))
            dec.advance()  # captures the step
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(new - 2):
                dec.advance()
            b.record()
            torch.cuda.synchronize()
            step = a.elapsed_time(b) / (new - 2)  # ms per replay
            print(json.dumps({"model": model, "kv_cache": kv or "bf16", "batch": B, "prompt": P, "round": rnd,
                              "new_tokens": dec.n_emitted, "cache_bytes": dec.cache.nbytes(),
                              "norm_fused_step": dec.norm_ws is not None, "ms_per_step": round(step, 3),
                              "decode_tokens_per_s": round(B / step * 1e3, 1)}), flush=True)
            del dec
            torch.cuda.empty_cache()


def kv_attn_main():
    """``DECODE_ATTN=1 DECODE_KV=fp8``: ``attn_decode`` (bf16 cache) against ``attn_decode_fp8``, batch 8,
    32 query / 8 kv heads, head_dim 128 and 64, 600 / 4,096 / 16,384 valid keys (a cache 64 slots
    longer), T = 1 and 4. Back-to-back launches timed with events, the arms alternating
    ``DECODE_ROUNDS`` (3) times; ``gbps`` counts the K + V (+ scale) bytes of the valid keys. Each arm
    rotates over enough copies of its cache that a launch finds none of its K / V in the 256 MiB
    last-level cache (``DECODE_ROTATE_MB``, default 1024, of cache bytes per arm; 0: one buffer,
    the cache-warm figure), as the layers of a model do."""
    from gke_ray_train_amd import _native
    from gke_ray_train_amd.ops import _ref
    C = _native.kernels()
    B, hq, hkv = 8, 32, 8

    rotate = int(os.environ.get("DECODE_ROTATE_MB", "1024")) << 20

    def timed(fn, bufs, iters):
        for i in range(10):
            fn(*bufs[i % len(bufs)])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(*bufs[i % len(bufs)])
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters * 1e3

    for D in (128, 64):
        bf = {1: C.attn_decode if D == 128 else C.attn_decode_d64,
              4: C.attn_decode_multi if D == 128 else C.attn_decode_multi_d64}
        f8 = C.attn_decode_fp8 if D == 128 else C.attn_decode_fp8_d64
        for n in (600, 4096, 16384):
            L = n + 64
            k = torch.randn(B, L, hkv, D, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(B, L, hkv, D, device="cuda", dtype=torch.bfloat16)
            (kc, ks), (vc, vs) = [[t.cuda() for t in _ref.kv_fp8_quantize(x.cpu())] for x in (k, v)]
            sl = torch.full((B,), n, device="cuda", dtype=torch.int32)
            bytes_bf, bytes_f8 = 2 * B * n * hkv * D * 2, 2 * B * n * hkv * (D + 4)
            bufs_b = [(k, v)] + [(k.clone(), v.clone()) for _ in range(-(-rotate // bytes_bf) - 1)]
            bufs_f = [(kc, vc, ks, vs)] + [tuple(t.clone() for t in (kc, vc, ks, vs))
                                           for _ in range(-(-rotate // bytes_f8) - 1)]
            iters = 200 if n <= 4096 else 50
            for T in (1, 4):
                q = torch.randn(B, T, hq, D, device="cuda", dtype=torch.bfloat16)
                for rnd in range(int(os.environ.get("DECODE_ROUNDS", "3"))):
                    us_b = timed(lambda k_, v_: bf[T](q, k_, v_, sl, D ** -0.5), bufs_b, iters)
                    us_f = timed(lambda *c: f8(q, *c, sl, D ** -0.5), bufs_f, iters)
                    print(json.dumps({"kernel": "attn_decode_fp8", "head_dim": D, "keys": n, "T": T, "round": rnd,
                                      "buffers": [len(bufs_b), len(bufs_f)],
                                      "bf16_us": round(us_b, 2), "fp8_us": round(us_f, 2),
                                      "bf16_gbps": round(bytes_bf / us_b / 1e3, 1),
                                      "fp8_gbps": round(bytes_f8 / us_f / 1e3, 1),
                                      "byte_ratio": round(bytes_f8 / bytes_bf, 3),
                                      "time_ratio": round(us_f / us_b, 3)}), flush=True)


if QUANT:
    nf4_main()
    sys.exit(0)
if "DECODE_KV" in os.environ:
    kv_attn_main() if "DECODE_ATTN" in os.environ else kv_main()
    sys.exit(0)
if "DECODE_SPEC" in os.environ:
    spec_main()
    sys.exit(0)
if "DECODE_ATTN" in os.environ:
    attn_main()
    sys.exit(0)
if "DECODE_SAMPLE" in os.environ or "DECODE_DEVICE_LOOP" in os.environ:
    sampler_main()
    sys.exit(0)
B = int(B_ENV)
m = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0)
ids = torch.randint(0, m.config.vocab_size, (B, 512), device="cuda")
from gke_ray_train_amd.ops import linear as _lin  # noqa: E402

runs = [(False, True), (True, False), (True, True)]  # (graph, gemv)
for mode, gemv in runs:
    _lin._GEMV = gemv
    m.generate(ids, max_new_tokens=8, use_graph=mode)  # warm-up (kernels, graph pools)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.generate(ids, max_new_tokens=128, use_graph=mode)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"model": model, "mode": ("hip_graph" if mode else "eager") + ("+gemv" if gemv else "+library_gemm"),
                      "batch": B, "new_tokens": out.shape[1] - 512,
                      "seconds": round(dt, 3), "tokens_per_s": round(B * (out.shape[1] - 512) / dt, 1)}), flush=True)
