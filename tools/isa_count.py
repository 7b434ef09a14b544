#!/usr/bin/env python3
"""Count instructions per kernel in a gfx950 assembly listing (hipcc --save-temps: *.s).

    python tools/isa_count.py build/isa/adamw8-hip-amdgcn-amd-amdhsa-gfx950.s [substring of the kernel name]

Per kernel: VALU (v_*), LDS (ds_*), vector memory (global_* / buffer_* / flat_*) and scalar (s_*)
instructions, for the whole function and per basic block (label to label), largest blocks first. The
hot loop of an element-wise kernel is its largest block, so "VALU per element" is that block's count
over the elements a lane handles per iteration. A static count: it says nothing about issue cycles.
"""
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return None


def main(path, want=""):
    kernel, block, stats = None, None, {}
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m:
            name = m.group(1)
            if not name.startswith(".L"):
                kernel = name
                stats[kernel] = {}
            block = name
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b", line)
        if not m or kernel is None:
            continue
        kind = classify(m.group(1))
        if kind:
            b = stats[kernel].setdefault(block, dict(valu=0, lds=0, vmem=0, salu=0))
            b[kind] += 1
    for k, blocks in stats.items():
        if want not in k or not blocks:
            continue
        tot = {x: sum(b[x] for b in blocks.values()) for x in ("valu", "lds", "vmem", "salu")}
        print(f"{k}\n  whole function: {tot}")
        for name, b in sorted(blocks.items(), key=lambda kv: -kv[1]["valu"])[:4]:
            print(f"  block {name}: {b}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
