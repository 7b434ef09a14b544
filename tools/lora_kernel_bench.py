#!/usr/bin/env python3
"""LoRA adapter kernels at the reference SFT job's shapes (Llama-3.1-8B, r = 64 on q/k/v/o/gate/up/down,
one packed step of T tokens): per module the grouped g = s dY B products (lora_g_group), the grouped
dB = dY^T h' token reductions (lora_tred_group), dA^T = x_d^T g (lora_tred, transposed) and the
dropout + down-projection h' = s drop(x) A^T (lora_down). Median of --reps launches per shape, with
the bytes of the big operand over time.

--rank 8 / 16 / 32 times the small-rank family instead (csrc/kernels/lora_small.hip) and, next to each
product, what the library path runs for it (``lib_*``: addmm_ per target, the dropout pass + GEMM,
GEMM + dropout backward), with the same one-read byte count of the big operand.

    python tools/lora_kernel_bench.py [--tokens 6144] [--reps 20] [--rank 64] [--tag name]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd import _native  # noqa: E402

H, I, KV = 4096, 14336, 1024
# module -> (input width, [target widths])
MODULES = {"qkv": (H, [H, KV, KV]), "o": (H, [H]), "gate_up": (H, [I, I]), "down": (I, [H])}


def timeit(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts)


def small_rank_arms(C, R, k, kin, x, xw, acat, dys, bts, gs, g, hs, dbs, dat, dy):
    """The lora_small.hip products of one module and the library calls they replace."""
    Rk = R * k
    bs = [b.t().contiguous() for b in bts]  # B_i [n_i, r], the library path's operand
    down = C.lora_small_down if Rk in (8, 16, 24, 48) else C.lora_down
    dx = torch.randn_like(x)
    at = acat.t().contiguous()

    def lib_g():
        for gj, dyj, b in zip(gs, dys, bs):
            gj.addmm_(dyj, b, beta=0.0, alpha=0.25)

    def lib_db():
        for db, dyj, h in zip(dbs, dys, hs):
            db.addmm_(dyj.t(), h, beta=0.0)

    def lib_down():
        xd = C.dropout_fwd_seeded(x, 0.1, 7, 0)
        xw[:, kin:].copy_((xd @ acat.t()) * 0.25)

    arms = {
        "small_g": (lambda: C.lora_small_g_group(dys, bts, gs, 0.25, False), dy.numel() * 2),
        "lib_g": (lib_g, dy.numel() * 2),
        "small_tred_dB": (lambda: C.lora_small_tred_group(dys, hs, dbs, 1.0, [False] * k), dy.numel() * 2),
        "lib_dB": (lib_db, dy.numel() * 2),
        "small_tred_dA": (lambda: (C.lora_small_tred if Rk % 64 else C.lora_tred)(x, g, dat, 1.0, False, True),
                          x.numel() * 2),
        "lib_dA": (lambda: dat.addmm_(g.t(), x, beta=0.0), x.numel() * 2),
        "down": (lambda: down(xw[:, :kin], acat, 0.1, 7, 0, True, h_out=xw[:, kin:], hscale=0.25), x.numel() * 2 * 2),
        "lib_down": (lib_down, x.numel() * 2 * 2),
    }
    if Rk % 16:
        arms["small_dx"] = (lambda: C.lora_small_dx(g, at, dx, 0.1, 7, 0, True), x.numel() * 2 * 2)
        arms["lib_dx"] = (lambda: C.dropout_bwd_seeded(g @ acat, dx, 0.1, 7, 0, True), x.numel() * 2 * 2)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=6144)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--rank", type=int, default=64, choices=[8, 16, 32, 64])
    a = ap.parse_args()
    R = a.rank
    C = _native.kernels()
    T = a.tokens
    dev = torch.device("cuda")
    torch.manual_seed(0)
    total = {}
    for name, (kin, ns) in MODULES.items():
        N = sum(ns)
        k = len(ns)
        dy = torch.randn(T, N, device=dev, dtype=torch.bfloat16)
        bt = torch.randn(R * k, N, device=dev, dtype=torch.bfloat16) * 0.05
        g = torch.empty(T, R * k, device=dev, dtype=torch.bfloat16)
        hc = torch.randn(T, R * k, device=dev, dtype=torch.bfloat16)
        x = torch.randn(T, kin, device=dev, dtype=torch.bfloat16)
        acat = torch.randn(R * k, kin, device=dev, dtype=torch.bfloat16) * 0.05
        offs = [sum(ns[:j]) for j in range(k)]
        dys = [dy[:, o:o + n] for o, n in zip(offs, ns)]
        bts = [bt[j * R:(j + 1) * R, o:o + n] for j, (o, n) in enumerate(zip(offs, ns))]
        gs = [g[:, j * R:(j + 1) * R] for j in range(k)]
        hs = [hc[:, j * R:(j + 1) * R] for j in range(k)]
        dbs = [torch.empty(n, R, device=dev, dtype=torch.bfloat16) for n in ns]
        dat = torch.empty(R * k, kin, device=dev, dtype=torch.bfloat16)
        xw = torch.empty(T, kin + R * k, device=dev, dtype=torch.bfloat16)
        xw[:, :kin] = x
        arms = {
            "lora_g": (lambda: C.lora_g_group(dys, bts, gs, 0.25, False), dy.numel() * 2),
            "tred_dB": (lambda: C.lora_tred_group(dys, hs, dbs, 1.0, [False] * k) if k > 1
                        else C.lora_tred(dys[0], hs[0], dbs[0], 1.0, False, False), dy.numel() * 2),
            "tred_dA": (lambda: C.lora_tred(x, g, dat, 1.0, False, True), x.numel() * 2),
            "lora_down": (lambda: C.lora_down(xw[:, :kin], acat, 0.1, 7, 0, True, h_out=xw[:, kin:], hscale=0.25),
                          x.numel() * 2 * 2),
        }
        if R < 64:
            arms = small_rank_arms(C, R, k, kin, x, xw, acat, dys, bts, gs, g, hs, dbs, dat, dy)
        for an, (fn, nbytes) in arms.items():
            fn()
            torch.cuda.synchronize()
            us = timeit(fn, a.reps)
            total[an] = total.get(an, 0.0) + us
            print(json.dumps({"tag": a.tag, "module": name, "kernel": an, "T": T, "us": round(us, 1),
                              "GBps": round(nbytes / us / 1e3, 1)}), flush=True)
    print(json.dumps({"tag": a.tag, "per_layer_us": {k: round(v, 1) for k, v in total.items()},
                      "per_layer_total_us": round(sum(total.values()), 1)}), flush=True)


if __name__ == "__main__":
    main()
