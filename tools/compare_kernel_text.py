#!/usr/bin/env python
"""Kernel by kernel, what changed between two gfx950 assembly listings of one source (hipcc <opt_amd/build.py FLAGS> -x hip --cuda-device-only -S, before and after
a change):  tools/compare_kernel_text.py <before.s> <after.s> [--all]

Kernels are matched by demangled name without the parameter list; comments are dropped and local labels renumbered.  Classes (profiles/graph_shared_text.md):
  a  the same instructions in the same order with the same registers
  b  the same opcode histogram and the same VGPRs / SGPRs / scratch / LDS / occupancy, in another order or with other register numbers
  c  anything else
Prints a markdown table (rocprim:: kernels as one line unless --all or not all of them are class a), then the kernels only one listing has.  Reads the two files and nothing else."""
import collections
import re
import subprocess
import sys

FUNC = re.compile(r"^(\S+):[ \t]*; @\1\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\t\.(?:globl|type|protected|weak|section\t\.text)|\Z)", re.S | re.M)
INFO = ("NumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    """{demangled name: [(instruction lines, resources), ...]} of the kernels (functions with a kernel descriptor) of one listing."""
    txt = open(path, errors="replace").read()
    found = []
    for m in FUNC.finditer(txt):
        sym, body, tail = m.groups()
        if ".amdhsa_kernel " + sym not in body:
            continue
        code = body.split("\t.section\t.rodata", 1)[0]
        lines = []
        for line in code.splitlines():
            line = line.split(";", 1)[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):      # comments, directives (labels stay)
                continue
            lines.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", line))            # .LBB<function number>_<block>: the function number is the listing's
        res = {k: int(v) for k, v in re.findall(r"^; (%s): (\d+)" % "|".join(INFO), tail, re.M)}
        found.append((sym, lines, res))
    names = subprocess.run(["c++filt"] + [f[0] for f in found], capture_output=True, text=True).stdout.splitlines()
    out = collections.defaultdict(list)
    for (sym, lines, res), n in zip(found, names):
        n = re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("optamd::", "").replace("void ", ""))
        out[n].append((lines, res))
    return out


def classify(a, b):
    if a[0] == b[0]:
        return "a"
    ops = lambda lines: collections.Counter(l.split()[0] for l in lines if not l.endswith(":"))
    return "b" if ops(a[0]) == ops(b[0]) and a[1] == b[1] else "c"


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    show_all = "--all" in sys.argv[3:]
    rows = []
    for n in sorted(set(before) & set(after)):
        assert len(before[n]) == len(after[n]), n
        for x, y in zip(before[n], after[n]):
            rows.append((n, classify(x, y), len(x[0]), len(y[0])))
    count = collections.Counter(c for _, c, _, _ in rows)
    print(f"{len(rows)} kernels in both listings: {count['a']} (a), {count['b']} (b), {count['c']} (c)\n")
    print("| kernel | class |\n|---|---|")
    lib = [r for r in rows if r[0].startswith("rocprim::")]
    fold = lib and not show_all and all(r[1] == "a" for r in lib)
    for n, c, la, lb in rows:
        if not (fold and n.startswith("rocprim::")):
            print(f"| `{n}` | {c}{'' if c == 'a' else f' ({la} -> {lb} instructions and labels)'} |")
    if fold:
        print(f"| the {len(lib)} `rocprim::` kernels | a |")
    for title, only in (("only in " + sys.argv[1], set(before) - set(after)), ("only in " + sys.argv[2], set(after) - set(before))):
        if only:
            print(f"\n{title}:")
            for n in sorted(only):
                print(f"- `{n}`")


if __name__ == "__main__":
    main()
