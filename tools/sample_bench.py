"""Isolated timing of the token sampler kernel (csrc/kernels/sample.hip) on MI355X: ``sample_logits`` on
bf16 logits [B, 128256] (the LM head's output in the decode step), B = 1 and 4, greedy / top-k 50 /
top-p 0.9 / both. One JSON line per case: microseconds per launch (device events around ``--iters``
back-to-back launches, after a warm-up), the passes over the row that mode makes and the implied
bytes/s = B * V * 2 bytes * passes / time. ``--torch`` adds the torch op chain the host loop of the
parent commit ran for the same choice (argmax, or softmax / sort / cumsum / scatter / multinomial)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd import _native  # noqa: E402

# passes over the row (sample.hip header): a 3-digit radix select per filter, a maximum pass for the
# masses of top-p, one final pass that draws
MODES = {
    "greedy": (dict(), 1),
    "temperature": (dict(do_sample=True, temperature=0.8), 1),
    "top_k50": (dict(do_sample=True, top_k=50), 4),
    "top_p0.9": (dict(do_sample=True, top_p=0.9), 5),
    "top_k50+top_p0.9": (dict(do_sample=True, top_k=50, top_p=0.9), 7),
}


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def torch_chain(logits, mode):
    if mode == "greedy":
        return logits.float().argmax(-1)
    probs = torch.softmax(logits.float(), -1)
    sp, si = probs.sort(-1, descending=True)
    keep = sp.cumsum(-1) - sp <= 0.9
    probs = torch.zeros_like(probs).scatter(-1, si, sp * keep)
    return torch.multinomial(probs / probs.sum(-1, keepdim=True), 1).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    K = _native.kernels()
    g = torch.Generator(device="cuda").manual_seed(0)
    counter = torch.zeros(1, dtype=torch.long, device="cuda")
    for rnd in range(a.rounds):
        for B in (1, 4):
            logits = (torch.randn(B, a.vocab, device="cuda", generator=g) * 4).bfloat16()
            for name, (kw, passes) in MODES.items():
                us = timed(lambda: K.sample_logits(logits, seed=1, counter=counter, **kw), a.iters)
                print(json.dumps({"kernel": "sample_logits", "mode": name, "B": B, "V": a.vocab, "round": rnd,
                                  "us": round(us, 2), "passes": passes,
                                  "GBps": round(B * a.vocab * 2 * passes / us / 1e3, 1)}), flush=True)
            if a.torch:
                for name in ("greedy", "top_p0.9"):
                    us = timed(lambda: torch_chain(logits, name), max(50, a.iters // 5))
                    print(json.dumps({"kernel": "torch ops", "mode": name, "B": B, "V": a.vocab, "round": rnd,
                                      "us": round(us, 2)}), flush=True)


if __name__ == "__main__":
    main()
