#!/usr/bin/env python3
"""bf16 flash-attention forward / backward timing (interleaved rounds, median) on random data at
the Llama-2-7B training shape (B8 S1024 H32 D128 causal) and a GQA shape, after a check against
the fp32 math reference (max abs error of O and of dQ / dK / dV). TFLOP/s count the algorithmic
causal FLOPs: 2 matmuls forward, 5 backward. The kernel generations compared in round 2
(profiles/r2_attention.md) were selected through a since-removed variant switch.
usage: python tools/attn_ab.py [--rounds 7]

--head-dim 64: the head_dim-64 bf16 kernels (attention_d64.hip) against the path they replaced,
the fp32 math attention (ops/_ref.attention and its autograd backward on the same GPU tensors), at
the two 64-wide training shapes: the gpt2-small BasicLLM step (B16 S256 H12 causal, dropout 0.1)
and the Llama-3.2-1B step (B8 S1024 Hq32 Hkv8 causal). Forward and forward + backward, interleaved
rounds after a warm-up, device events; median, min and max per variant, and for information the
D = 128 kernels at the same B, S, H.

--head-dim 64 --rope [--packed L1,L2,...]: ``ops.rope_attention`` at Hq32 Hkv8 on the qkv-native
kernels (attention_d64.hip, FusedRope policy) against the path they replace (GRT_ROPE_ATTN_D64=0 semantics: torch
RoPE, then the flash kernels, one call per sequence when packed), unpacked B8 S1024 or the packed
lengths; same protocol, both arms checked against the fp32 math path first.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd import _native  # noqa: E402
from gke_ray_train_amd.ops import _ref  # noqa: E402

C = _native.kernels()
SCHEDS = ""


def ev_time(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3  # us


def run(shape, rounds, iters):
    B, S, Hq, Hkv = shape
    D = 128
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    do = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
    scale = D ** -0.5
    flop_mm = 2 * B * Hq * S * S * D / 2  # one causal matmul
    # reference on a slice of heads (fp32 math path)
    hs = slice(0, min(Hq, 4))
    kv_hs = slice(0, max(1, (min(Hq, 4) * Hkv) // Hq))
    qr, kr, vr = (t.float().requires_grad_() for t in (q[:, :, hs], k[:, :, kv_hs], v[:, :, kv_hs]))
    orf = _ref.attention(qr, kr, vr, causal=True, scale=scale)
    orf.backward(do[:, :, hs].float())
    out = {}
    o, lse = C.attn_fwd(q, k, v, None, scale, True, None)
    out["fwd"] = {"max_err": (o[:, :, hs].float() - orf.detach()).abs().max().item(), "t": []}
    dq, dk, dv = C.attn_bwd(do, q, k, v, o, lse, None, None, None, scale, True, None)
    out["bwd"] = {"max_err_dq_dk_dv": [(dq[:, :, hs].float() - qr.grad).abs().max().item(),
                                       (dk[:, :, kv_hs].float() - kr.grad).abs().max().item() if Hq == Hkv else None,
                                       (dv[:, :, kv_hs].float() - vr.grad).abs().max().item() if Hq == Hkv else None],
                  "t": []}
    scheds = [int(x) for x in SCHEDS.split(",")] if SCHEDS else [None]
    if len(scheds) > 1:  # every schedule must give bitwise the same outputs (same per-block math)
        res = []
        for sc in scheds:
            C.attn_set_schedule(sc)
            o_s, lse_s = C.attn_fwd(q, k, v, None, scale, True, None)
            res.append((o_s, lse_s, *C.attn_bwd(do, q, k, v, o_s, lse_s, None, None, None, scale, True, None)))
        for sc, r in zip(scheds[1:], res[1:]):
            same = all(torch.equal(x, y) for x, y in zip(res[0], r))
            print(json.dumps({"shape": f"B{B} S{S} Hq{Hq} Hkv{Hkv}", "sched": sc, "bitwise_equal_to": scheds[0],
                              "equal": same}), flush=True)
    for sc in scheds:
        for name in ("fwd", "bwd"):
            out.setdefault(f"{name}_s{sc}", {"t": []}) if sc is not None else None
    for _ in range(rounds):
        for sc in scheds:
            if sc is not None:
                C.attn_set_schedule(sc)
            kf, kb = ("fwd", "bwd") if sc is None else (f"fwd_s{sc}", f"bwd_s{sc}")
            out[kf]["t"].append(ev_time(lambda: C.attn_fwd(q, k, v, o, scale, True, None), iters))
            out[kb]["t"].append(ev_time(
                lambda: C.attn_bwd(do, q, k, v, o, lse, None, None, None, scale, True, None), iters))
    if scheds[0] is not None:
        del out["fwd"]["t"], out["bwd"]["t"]
        out["fwd"]["t"], out["bwd"]["t"] = [], []
        out = {k: v for k, v in out.items() if v["t"]} | {k: out[k] for k in ("fwd", "bwd")}
    for name, r in out.items():
        if not r.get("t"):
            r.pop("t", None)
            print(json.dumps({"shape": f"B{B} S{S} Hq{Hq} Hkv{Hkv} D128 causal", "kernel": name, **r}), flush=True)
            continue
        t = statistics.median(r.pop("t"))
        nmm = 2 if name.startswith("fwd") else 5
        r.update(us=round(t, 1), tflops=round(nmm * flop_mm / t / 1e6, 1))
        print(json.dumps({"shape": f"B{B} S{S} Hq{Hq} Hkv{Hkv} D128 causal", "kernel": name, **r}), flush=True)


def run_d64(shape, dropout_p, rounds, iters):
    B, S, Hq, Hkv = shape
    g = torch.Generator(device="cuda").manual_seed(0)

    def mk(D):
        return [torch.randn(B, S, h, D, device="cuda", dtype=torch.bfloat16, generator=g) for h in (Hq, Hkv, Hkv, Hq)]
    q, k, v, do = mk(64)
    q2, k2, v2, do2 = mk(128)
    qr, kr, vr = (t.detach().clone().requires_grad_() for t in (q, k, v))
    seed = 1234

    def kern_fwd(q=q, k=k, v=v, D=64):
        return C.attn_fwd(q, k, v, None, D ** -0.5, True, None, dropout_p, seed)

    def kern_fb(q=q, k=k, v=v, do=do, D=64):
        o, lse = C.attn_fwd(q, k, v, None, D ** -0.5, True, None, dropout_p, seed)
        return C.attn_bwd(do, q, k, v, o, lse, None, None, None, D ** -0.5, True, None, dropout_p, seed)

    def ref_fwd():
        return _ref.attention(qr, kr, vr, causal=True, dropout_p=dropout_p, seed=seed)

    def ref_fb():
        for t in (qr, kr, vr):
            t.grad = None
        ref_fwd().backward(do)

    variants = {
        "d64_fwd": kern_fwd, "d64_fwd_bwd": kern_fb, "math_fwd": ref_fwd, "math_fwd_bwd": ref_fb,
        "d128_fwd": lambda: kern_fwd(q2, k2, v2, 128), "d128_fwd_bwd": lambda: kern_fb(q2, k2, v2, do2, 128),
    }
    # agreement of the two timed paths before timing them
    o, _ = kern_fwd()
    dq, dk, dv = kern_fb()
    ref_fb()
    err = {"o": (o.float() - ref_fwd().detach().float()).abs().max().item(),
           "dq": (dq.float() - qr.grad.float()).abs().max().item(),
           "dk": (dk.float() - kr.grad.float()).abs().max().item(),
           "dv": (dv.float() - vr.grad.float()).abs().max().item()}
    for fn in variants.values():  # warm-up
        ev_time(fn, 2)
    ts = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            ts[n].append(ev_time(fn, iters))
    name = f"B{B} S{S} Hq{Hq} Hkv{Hkv} causal dropout {dropout_p}"
    print(json.dumps({"shape": name, "max_abs_err_vs_math": err}), flush=True)
    flop_mm = 2 * B * Hq * S * S / 2  # one causal matmul, per unit of head_dim
    st = {}
    for n, t in ts.items():
        D = 128 if n.startswith("d128") else 64
        nmm = 2 if n.endswith("_fwd") else 7
        st[n] = dict(us=round(statistics.median(t), 1), min=round(min(t), 1), max=round(max(t), 1),
                     tflops=round(nmm * flop_mm * D / statistics.median(t) / 1e6, 1))
        print(json.dumps({"shape": name, "variant": n, **st[n]}), flush=True)
    for part in ("fwd", "fwd_bwd"):
        a, b = st[f"d64_{part}"], st[f"math_{part}"]
        spread = (a["max"] - a["min"]) + (b["max"] - b["min"])
        print(json.dumps({"shape": name, "part": part, "speedup": round(b["us"] / a["us"], 2),
                          "gain_us": round(b["us"] - a["us"], 1), "spread_us": round(spread, 1),
                          "faster_beyond_spread": b["us"] - a["us"] > spread}), flush=True)


def run_rope_d64(B, S, lens, rounds, iters, Hq=32, Hkv=8):
    """``ops.rope_attention`` at head_dim 64, qkv-native kernels (attention_d64.hip, FusedRope policy) against the
    path they replace (GRT_ROPE_ATTN_D64=0: torch RoPE, then the flash kernels, one call per
    sequence when packed). ``lens``: packed sequence lengths, or None for B sequences of S rows."""
    from gke_ray_train_amd import ops
    from gke_ray_train_amd.ops import fused
    D = 64
    g = torch.Generator(device="cuda").manual_seed(0)
    vl = ops.Varlen(lens, torch.device("cuda", 0)) if lens else None
    if vl is not None:
        B, S = 1, vl.total
    T = B * S
    rows = vl.max_len if vl is not None else S
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16, generator=g).requires_grad_()
    do = torch.randn(T, Hq * D, device="cuda", dtype=torch.bfloat16, generator=g)
    cos, sin = _ref.rope_tables(rows, D, device="cuda")

    def call(new, bwd):
        fused._ROPE_ATTN_D64 = new
        qkv.grad = None
        o = ops.rope_attention(qkv, cos, sin, B, S, Hq, Hkv, D, causal=True, varlen=vl)
        if bwd:
            o.backward(do)
        return o

    variants = {"new_fwd": lambda: call(True, False), "new_fwd_bwd": lambda: call(True, True),
                "parent_fwd": lambda: call(False, False), "parent_fwd_bwd": lambda: call(False, True)}
    # both arms against the fp32 math path, sequence by sequence
    x = qkv.detach().float().requires_grad_()
    xr = x.view(T, Hq + 2 * Hkv, D)
    pos = vl.pos if vl is not None else torch.arange(T, device="cuda") % S
    bounds = list(zip(vl.cu_host[:-1], vl.cu_host[1:])) if vl is not None else [(b * S, (b + 1) * S) for b in range(B)]
    qr, kr = (_ref.apply_rope(xr[:, a:b], cos, sin, pos) for a, b in ((0, Hq), (Hq, Hq + Hkv)))
    vr = xr[:, Hq + Hkv:]
    ref = torch.cat([_ref.attention(qr[a:b].unsqueeze(0), kr[a:b].unsqueeze(0), vr[a:b].unsqueeze(0), causal=True)[0]
                     for a, b in bounds]).reshape(T, Hq * D)
    ref.backward(do.float())
    err = {}
    for arm, new in (("new", True), ("parent", False)):
        o = call(new, True)
        err[arm] = {"o": (o.float() - ref.detach()).abs().max().item(),
                    "dqkv": (qkv.grad.float() - x.grad).abs().max().item()}
    name = (f"packed {','.join(map(str, lens))}" if lens else f"B{B} S{S}") + f" Hq{Hq} Hkv{Hkv} D64 causal rope"
    print(json.dumps({"shape": name, "max_abs_err_vs_math": err}), flush=True)
    del x, xr, qr, kr, vr, ref
    for fn in variants.values():  # warm-up
        ev_time(fn, 2)
    ts = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            ts[n].append(ev_time(fn, iters))
    fused._ROPE_ATTN_D64 = True
    st = {}
    for n, t in ts.items():
        st[n] = dict(us=round(statistics.median(t), 1), min=round(min(t), 1), max=round(max(t), 1))
        print(json.dumps({"shape": name, "variant": n, **st[n]}), flush=True)
    for part in ("fwd", "fwd_bwd"):
        a, b = st[f"new_{part}"], st[f"parent_{part}"]
        spread = (a["max"] - a["min"]) + (b["max"] - b["min"])
        print(json.dumps({"shape": name, "part": part, "speedup": round(b["us"] / a["us"], 2),
                          "gain_us": round(b["us"] - a["us"], 1), "spread_us": round(spread, 1),
                          "faster_beyond_spread": b["us"] - a["us"] > spread,
                          "slower_beyond_spread": a["us"] - b["us"] > spread}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scheds", default="", help="comma-separated workgroup schedules to A/B (attn_set_schedule)")
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128),
                    help="64: the head_dim-64 kernels against the fp32 math path they replaced")
    ap.add_argument("--rope", action="store_true",
                    help="with --head-dim 64: ops.rope_attention, qkv-native kernels against GRT_ROPE_ATTN_D64=0")
    ap.add_argument("--packed", default="", help="with --rope: comma-separated packed sequence lengths "
                    "(default: unpacked B8 S1024)")
    a = ap.parse_args()
    SCHEDS = a.scheds
    if a.rope or a.packed:
        if a.head_dim != 64 or not a.rope:
            ap.error("--rope / --packed measure the head_dim-64 op: use --head-dim 64 --rope [--packed L1,L2,...]")
        run_rope_d64(8, 1024, [int(x) for x in a.packed.split(",")] if a.packed else None, a.rounds, a.iters)
        sys.exit(0)
    if a.head_dim == 64:
        run_d64((16, 256, 12, 12), 0.1, a.rounds, a.iters)
        run_d64((8, 1024, 32, 8), 0.0, a.rounds, a.iters)
        sys.exit(0)
    for shape in ((8, 1024, 32, 32), (2, 2048, 32, 8)):
        run(shape, a.rounds, a.iters)
