#!/usr/bin/env python3
"""Compare the gfx950 code of kernels in two .hip files, symbol by symbol, without a GPU.

For a refactor that must not change what runs: compile the old and the new file with the device
flags of gke_ray_train_amd/_build.py, split the assembly per kernel, drop comments and directives,
renumber the ``.LBBn_m`` labels (n is the function's index in its file) and compare the instruction
lists line by line. Per pair: instruction count, identical or not, and the register / scratch / LDS
figures of both sides from the code-object metadata; where the streams differ, the opcodes whose
counts differ.

usage: python tools/isa_diff.py OLD.hip NEW.hip OLD_SUBSTRING=NEW_SUBSTRING [...]
       (OLD.hip may be several files joined by commas)

A substring is looked for in the mangled and in the demangled kernel name and must select exactly
one kernel of its side. Exit status 1 if any pair differs in its stream or its figures.
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "gke_ray_train_amd" / "csrc" / "include"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-munsafe-fp-atomics"]
FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def assembly(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, *FLAGS, "-I", str(INCLUDE), "--cuda-device-only", "-S", str(src), "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{src}: compile failed\n{r.stderr}")
    return r.stdout


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"
    try:
        out = subprocess.run([filt, *names], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(asm):
    """{symbol: {"insts": [...], figure: int, ...}} for every kernel of one assembly file."""
    meta = {}
    for block in re.split(r"^  - (?=\.)", asm, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, flags=re.M)
        if not name or ".vgpr_count" not in block:
            continue
        meta[name.group(1)] = {f: int(re.search(rf"^\s*{re.escape(f)}:\s*(\d+)", block, flags=re.M).group(1))
                               for f in FIGURES}
    lines = [line.split(";")[0].strip() for line in asm.split("\n")]
    out = {}
    for sym, figures in meta.items():
        start = lines.index(sym + ":")
        insts = []
        for line in lines[start + 1:]:
            if line.startswith(".Lfunc_end"):
                break
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue
            insts.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))
        out[sym] = {"insts": insts, **figures}
    return out


def pick(table, names, sub, side):
    hits = [s for s in table if sub in s or sub in names[s]]
    if len(hits) != 1:
        listing = "\n  ".join(names[s] for s in (hits or table))
        sys.exit(f"{side}: '{sub}' selects {len(hits)} kernels; " + ("matches" if hits else "kernels") + f":\n  {listing}")
    return hits[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("pairs", nargs="+", metavar="OLD_SUBSTRING=NEW_SUBSTRING")
    a = ap.parse_args()
    old = {}
    for f in a.old.split(","):
        old.update(kernels(assembly(f)))
    new = kernels(assembly(a.new))
    names = demangle([*old, *new])
    print("| old = new | instructions | stream | VGPRs | SGPRs | scratch bytes | LDS bytes |")
    print("|---|---|---|---|---|---|---|")
    differ, notes = False, []
    for pair in a.pairs:
        so, sn = pair.split("=", 1)
        ko, kn = old[pick(old, names, so, "old")], new[pick(new, names, sn, "new")]
        same = ko["insts"] == kn["insts"]
        figs = [str(ko[f]) if ko[f] == kn[f] else f"{ko[f]} -> {kn[f]}" for f in FIGURES]
        n = str(len(ko["insts"])) if len(ko["insts"]) == len(kn["insts"]) else f"{len(ko['insts'])} -> {len(kn['insts'])}"
        print(f"| {so} = {sn} | {n} | {'identical' if same else 'DIFFERS'} | " + " | ".join(figs) + " |")
        differ |= not same or any(ko[f] != kn[f] for f in FIGURES)
        if not same:
            co = collections.Counter(i.split()[0] for i in ko["insts"] if not i.endswith(":"))
            cn = collections.Counter(i.split()[0] for i in kn["insts"] if not i.endswith(":"))
            d = {op: cn[op] - co[op] for op in sorted({*co, *cn}) if cn[op] != co[op]}
            first = next((i for i, (x, y) in enumerate(zip(ko["insts"], kn["insts"])) if x != y),
                         min(len(ko["insts"]), len(kn["insts"])))
            notes.append(f"{so} = {sn}: first difference at instruction {first}; opcode counts new - old: "
                         + (", ".join(f"{op} {v:+d}" for op, v in d.items()) or "none (same opcodes, other order or operands)"))
    print("\n".join(["", *notes]) if notes else "")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
