"""DoRA measurements (profiles/dora.md).

``python tools/bench_dora.py kernel`` times the norm kernel of csrc/kernels/dora.hip alone at the
Llama-3.1-8B projection shapes, bf16 and NF4 weights, against the obvious alternative (dequantise for
NF4, then addmm + linalg.norm on the materialised W + s B A); the arms alternate in one process and
each figure is the median of the rounds. GB/s counts the weight bytes read.

``python tools/bench_dora.py step -- <bench.py arguments>`` runs bench.py's workload unchanged except
that every LoraConfig it builds has use_dora=True, and adds the HBM peak to the JSON line."""
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("qkv", 6144, 4096, [(0, 4096), (4096, 1024), (5120, 1024)]), ("o", 4096, 4096, [(0, 4096)]),
          ("gate_up", 28672, 4096, [(0, 14336), (14336, 14336)]), ("down", 4096, 14336, [(0, 4096)])]


def _time(fn, iters=5):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters * 1e3  # us


def kernel(r=64, rounds=7):
    from gke_ray_train_amd import _native
    from gke_ray_train_amd.peft import BitsAndBytesConfig
    from gke_ray_train_amd.peft.quant import NF4Linear
    C = _native.kernels()
    dev, bf, s = "cuda", torch.bfloat16, 0.25
    for name, out, K, targets in SHAPES:
        lin = torch.nn.Linear(K, out, bias=False, device=dev, dtype=bf)
        layer = NF4Linear.from_linear(lin, BitsAndBytesConfig())
        As = [torch.randn(r, K, device=dev, dtype=bf) * 0.02 for _ in targets]
        Bs = [torch.randn(n, r, device=dev, dtype=bf) * 0.02 for _, n in targets]
        Ms = [torch.ones(n, device=dev, dtype=bf) for _, n in targets]
        offs = [o for o, _ in targets]
        w = lin.weight.detach()

        def direct(wt):
            for (off, n), a, b in zip(targets, As, Bs):
                torch.linalg.norm(torch.addmm(wt[off:off + n], b, a, alpha=s), dim=1)

        arms = {"bf16 kernel": lambda: C.dora_norm(w, None, None, As, Bs, Ms, offs, out, s, False),
                "bf16 addmm+norm": lambda: direct(w),
                "nf4 kernel": lambda: C.dora_norm(None, layer.qweight, layer.absmax, As, Bs, Ms, offs, out, s, False),
                "nf4 dequant+addmm+norm": lambda: direct(layer._dequant())}
        times = {k: [] for k in arms}
        for rd in range(rounds + 1):
            for k, fn in arms.items():
                t = _time(fn)
                if rd:  # round 0 warms up
                    times[k].append(t)
        for k, v in times.items():
            med = statistics.median(v)
            nbytes = out * K * (0.5 + 4 / 64 if k.startswith("nf4") else 2)
            print(json.dumps({"shape": name, "out": out, "in": K, "r": r, "arm": k, "us": round(med, 1),
                              "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                              "weight_GBps": round(nbytes / med / 1e3, 1)}), flush=True)


def step(argv):
    import bench
    import gke_ray_train_amd.peft as peft
    peft.LoraConfig = functools.partial(peft.LoraConfig, use_dora=True)
    sys.argv = ["bench.py"] + argv
    try:
        bench.main()
    finally:
        print(json.dumps({"use_dora": True, "hbm_peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        kernel()
    elif len(sys.argv) > 2 and sys.argv[1] == "step" and sys.argv[2] == "--":
        step(sys.argv[3:])
    else:
        sys.exit(__doc__)
