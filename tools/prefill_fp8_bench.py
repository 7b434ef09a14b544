"""Chunked prefill attention over the fp8 KV cache on MI355X: the flash kernel that reads the codes
(``ops.prefill_attention_fp8``, prefill_attention_fp8.hip) against the path it replaces (two
``kv_fp8_dequant`` launches writing a bf16 copy of rows [0, n), then ``flash_attention`` on the
copies) and against ``flash_attention`` on a bf16 cache of the same shape (the reference point).

One chunk of S = 512 query tokens on n = 512 / 4,096 / 32,768 keys, batch 1, 32 query / 8 kv heads,
head_dim 128 (the 8B model) and 64 (the 1B model), a cache 64 slots longer than n. Back-to-back
launches timed with device events after a warm-up, the three arms alternating ``PREFILL_ROUNDS`` (3)
times in this one process; each arm rotates over copies of its cache that add up to
``PREFILL_ROTATE_MB`` (1024) so that a launch finds its K / V in HBM, as a model's layers do. One
JSON line per shape and round: microseconds per call, the bytes each arm has to move (computed
from the shapes: codes + scales or bf16 rows once, q and o once, the parent's copy written and read
back) and max |new - parent| of the outputs."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd import _native, ops  # noqa: E402
from gke_ray_train_amd.ops import _ref  # noqa: E402

B, S, HQ, HKV = 1, 512, 32, 8
ROUNDS = int(os.environ.get("PREFILL_ROUNDS", "3"))
ROTATE = int(os.environ.get("PREFILL_ROTATE_MB", "1024")) << 20
KEYS = [int(n) for n in os.environ.get("PREFILL_KEYS", "512,4096,32768").split(",")]


def timed(fn, bufs, iters):
    for i in range(5):
        fn(*bufs[i % len(bufs)])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(*bufs[i % len(bufs)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def copies(first, nbytes):
    return [first] + [tuple(t.clone() for t in first) for _ in range(-(-ROTATE // nbytes) - 1)]


def main():
    if not torch.cuda.is_available():
        sys.exit("prefill_fp8_bench: needs the GPU")
    C = _native.kernels()
    for D in (128, 64):
        for n in KEYS:
            L = n + 64
            g = torch.Generator().manual_seed(n + D)
            k, v = (torch.randn(B, L, HKV, D, generator=g).bfloat16() for _ in range(2))
            (kc, ks), (vc, vs) = ([t.cuda() for t in _ref.kv_fp8_quantize(x)] for x in (k, v))
            k, v = k.cuda(), v.cuda()
            q = torch.randn(B, S, HQ, D, generator=g).bfloat16().cuda()
            qo = 2 * B * S * HQ * D * 2
            kv_f8, kv_bf = 2 * B * n * HKV * (D + 4), 2 * B * n * HKV * D * 2
            bytes_ = {"new": qo + kv_f8, "parent": qo + kv_f8 + 2 * kv_bf, "bf16": qo + kv_bf}
            bufs_f = copies((kc, vc, ks, vs), kv_f8)
            bufs_b = copies((k, v), kv_bf)

            def new(kc_, vc_, ks_, vs_):
                return ops.prefill_attention_fp8(q, kc_[:, :n], vc_[:, :n], ks_[:, :n], vs_[:, :n])

            def parent(kc_, vc_, ks_, vs_):
                return ops.flash_attention(q, C.kv_fp8_dequant(kc_, ks_, n), C.kv_fp8_dequant(vc_, vs_, n), causal=True)

            def bf16(k_, v_):
                return ops.flash_attention(q, k_[:, :n], v_[:, :n], causal=True)

            diff = (new(*bufs_f[0]).float() - parent(*bufs_f[0]).float()).abs().max().item()
            iters = 100 if n <= 4096 else 30
            for rnd in range(ROUNDS):
                us = {"new": timed(new, bufs_f, iters), "parent": timed(parent, bufs_f, iters),
                      "bf16": timed(bf16, bufs_b, iters)}
                print(json.dumps({"kernel": "attn_prefill_fp8", "head_dim": D, "S": S, "keys": n, "round": rnd,
                                  "buffers": [len(bufs_f), len(bufs_b)],
                                  **{f"{a}_us": round(t, 1) for a, t in us.items()},
                                  **{f"{a}_mb": round(bytes_[a] / 1e6, 2) for a in us},
                                  "new_over_parent": round(us["new"] / us["parent"], 3),
                                  "new_over_bf16": round(us["new"] / us["bf16"], 3),
                                  "max_abs_new_minus_parent": round(diff, 5)}), flush=True)
            del bufs_f, bufs_b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
