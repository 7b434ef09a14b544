"""One masked batch of two prompts of unequal length against two single-prompt ``generate`` calls
(models/generation.py). Random init, bf16, greedy, HIP-graph decode; the two arms alternate
``RAGGED_ROUNDS`` (3) times in this one process, each timed call after a warm-up call of the same
shapes, the host clock around a device synchronise. One JSON line per arm and round.

``python tools/ragged_generate_bench.py [model] [len_a,len_b] [new_tokens]`` (llama3.2-1b, 200,700, 128)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gke_ray_train_amd.models import build_llama  # noqa: E402

model = sys.argv[1] if len(sys.argv) > 1 else "llama3.2-1b"
lens = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "200,700").split(",")]
new = int(sys.argv[3]) if len(sys.argv) > 3 else 128
m = build_llama(model, device="cuda", dtype=torch.bfloat16, seed=0).eval()
g = torch.Generator(device="cuda").manual_seed(0)
prompts = [torch.randint(0, m.config.vocab_size, (n,), device="cuda", generator=g) for n in lens]
S = max(lens)
ids = torch.zeros(len(lens), S, dtype=torch.long, device="cuda")
mask = torch.zeros_like(ids)
for b, p in enumerate(prompts):  # left-padded, pad id 0
    ids[b, S - len(p):] = p
    mask[b, S - len(p):] = 1


def batch():
    return m.generate(ids, attention_mask=mask, max_new_tokens=new)[:, S:]


def singles():
    return torch.stack([m.generate(p[None], max_new_tokens=new)[0, len(p):] for p in prompts])


def timed(fn):
    fn()  # warm-up: kernels, graph pools, the shapes of this arm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for rnd in range(int(os.environ.get("RAGGED_ROUNDS", "3"))):
    res = {}
    for name, fn in (("two_single_calls", singles), ("one_masked_batch", batch)):
        dt, res[name] = timed(fn)
        print(json.dumps({"model": model, "arm": name, "round": rnd, "prompt_lens": lens, "new_tokens": new,
                          "seconds": round(dt, 4), "tokens_per_s": round(len(lens) * new / dt, 1)}), flush=True)
    same = (res["two_single_calls"] == res["one_masked_batch"]).float().mean(1).tolist()
    print(json.dumps({"round": rnd, "fraction_of_tokens_equal_per_row": [round(x, 3) for x in same]}), flush=True)
