#!/usr/bin/env python3
"""adamw (fp32 moments) against adamw8 (8-bit block-quantised moments) on one GPU.

    python tools/bench_adamw8.py [--log2n 27] [--rounds 15] [--launches 40] [--max-blocks 0] [--out FILE.json]

Both kernels update the same 2^log2n bf16 parameters from the same bf16 gradient (no master copy,
stochastic rounding on: the configuration of the headline step). The arms are interleaved: each
round times `launches` back-to-back launches of one arm, then of the other, between two device
events, so drift of the clock or of a shared host hits both alike. The moments are brought to a
realistic state first (a few steps on changing random gradients), every timed shape is warmed up,
and the two parameter copies are compared after the warm-up (8-bit moments change the update a
little; a large difference would mean a broken kernel, not a faster one).

Bytes per element are what the algorithm has to move, from the shapes: adamw 22 (p 2+2, g 2, m 4+4,
v 4+4), adamw8 10 + 16/256 (p 2+2, g 2, codes 1+1 and 1+1, two absmax read and written per block).
Achieved TB/s is those bytes over the median time per launch. There is no fallback: without a GPU
and the built kernels this fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BYTES = {"adamw": 22.0, "adamw8": 10.0 + 16.0 / 256.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--prep-steps", type=int, default=3)
    ap.add_argument("--max-blocks", type=int, default=0, help="grid cap of the adamw8 launches (0: the kernel's own)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adamw8: no GPU")
    from gke_ray_train_amd import _native
    from gke_ray_train_amd.ops import _ref
    C = _native.kernels()
    dev = "cuda"
    n = 1 << a.log2n
    gen = torch.Generator(device=dev).manual_seed(0)
    p0 = (0.02 * torch.randn(n, device=dev, generator=gen)).to(torch.bfloat16)
    g = torch.empty(n, device=dev, dtype=torch.bfloat16)
    state = {
        "adamw": dict(p=p0.clone(), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev)),
        "adamw8": dict(p=p0.clone(),
                       cm=torch.full((n,), _ref.Q8_ZERO_CODE[True], dtype=torch.uint8, device=dev),
                       am=torch.zeros(n // 256, device=dev),
                       cv=torch.full((n,), _ref.Q8_ZERO_CODE[False], dtype=torch.uint8, device=dev),
                       av=torch.zeros(n // 256, device=dev)),
    }
    hyper = torch.empty(10, device=dev)
    step = [0]

    def set_step():
        step[0] += 1
        s = step[0]
        hyper.copy_(torch.tensor([2e-5, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** s, 1 - 0.999 ** s, 1.0, 1.0, float(s)]))

    def launch(arm):
        st = state[arm]
        if arm == "adamw":
            C.adamw(st["p"], g, st["m"], st["v"], None, hyper, None, 0, 0)
        else:
            C.adamw8(st["p"], g, st["cm"], st["am"], st["cv"], st["av"], None, hyper, None, a.max_blocks, 0)

    for _ in range(a.prep_steps):  # realistic moments, and the warm-up of both shapes
        g.copy_((1e-3 * torch.randn(n, device=dev, generator=gen) *
                 torch.exp(torch.randn(n, device=dev, generator=gen))).to(torch.bfloat16))
        set_step()
        for arm in state:
            launch(arm)
    torch.cuda.synchronize()
    diff = (state["adamw"]["p"].float() - state["adamw8"]["p"].float()).abs()
    m8 = torch.empty(n, device=dev)
    C.dequantize_blockwise8(state["adamw8"]["cm"], state["adamw8"]["am"], m8, True)
    m_err = ((m8 - state["adamw"]["m"]).abs().mean() / state["adamw"]["m"].abs().mean()).item()
    del m8
    times = {arm: [] for arm in state}
    for r in range(a.rounds):
        set_step()
        for arm in (("adamw", "adamw8") if r % 2 == 0 else ("adamw8", "adamw")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch(arm)
            e1.record()
            e1.synchronize()
            times[arm].append(e0.elapsed_time(e1) * 1e3 / a.launches)  # us per launch
    res = {"n": n, "adamw8_max_blocks": a.max_blocks, "rounds": a.rounds, "launches_per_round": a.launches, "device": torch.cuda.get_device_name(0),
           "p_max_abs_diff_after_prep": diff.max().item(), "m_mean_rel_err_after_prep": m_err, "arms": {}}
    for arm, t in times.items():
        med = statistics.median(t)
        res["arms"][arm] = {"us_per_launch_median": med, "us_min": min(t), "us_max": max(t),
                            "bytes_per_element": BYTES[arm], "achieved_TBps": BYTES[arm] * n / (med * 1e-6) / 1e12}
    res["time_ratio_adamw8_over_adamw"] = res["arms"]["adamw8"]["us_per_launch_median"] / res["arms"]["adamw"]["us_per_launch_median"]
    res["byte_ratio_adamw8_over_adamw"] = BYTES["adamw8"] / BYTES["adamw"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
