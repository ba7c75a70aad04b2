#!/usr/bin/env python3
"""Per-kernel resource usage and instruction counts of two builds, side by side: what a source change did to the code
generation, read from compiler output alone (no GPU).

A build directory holds, per source NAME.hip compiled with the Makefile's flags plus
`-Rpass-analysis=kernel-resource-usage -save-temps`, the compiler's stderr in NAME.log and the device assembly NAME-hip-*.s:
    cd <dir> && hipcc $HIPFLAGS -Rpass-analysis=kernel-resource-usage -save-temps -c <csrc>/NAME.hip -o NAME.o 2> NAME.log
Usage: kernel_resources.py <dir A> <dir B> [--all] > profiles/<name>.md
Prints the compiler's version string, one table row per kernel that differs (every kernel with --all), and the kernels that
exist in only one of the two builds."""
import glob
import os
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]
SHORT = ["VGPR", "AGPR", "SGPR", "scratch", "VGPR spill", "SGPR spill", "LDS", "occupancy", "instructions"]
REMARK = re.compile(r"remark: .*?:\d+:\d+:\s+(.+?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def read_build(d):
    """{demangled kernel: [the FIELDS..., instructions]} and the compiler's .ident string"""
    res, cur = {}, None
    for log in sorted(glob.glob(os.path.join(d, "*.log"))):
        for line in open(log, errors="replace"):
            m = REMARK.match(line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None and m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
    ident = ""
    for asm in sorted(glob.glob(os.path.join(d, "*-hip-amdgcn-*.s"))):
        name = None
        for line in open(asm, errors="replace"):
            if name is None:
                m = re.match(r"(\w+):", line)
                if m and m.group(1) in res:
                    name, n = m.group(1), 0
                elif line.startswith("\t.ident"):
                    ident = line.split('"')[1]
            elif line.startswith(".Lfunc_end"):
                res[name]["instructions"] = n
                name = None
            elif line.startswith("\t") and line[1] not in ".;\n":     # an instruction: not a directive, comment or label
                n += 1
    names = list(res)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = [re.sub(r"\(anonymous namespace\)::|ddsp_osc::|^void |\(.*\)$", "", p) for p in plain]
    return {s: [res[n].get(f, -1) for f in FIELDS + ["instructions"]] for s, n in zip(short, names)}, ident


def main():
    dirs = [a for a in sys.argv[1:] if not a.startswith("--")]
    (a, ident_a), (b, ident_b) = read_build(dirs[0]), read_build(dirs[1])
    print(f"compiler A: {ident_a}\n\ncompiler B: {ident_b}\n")
    both = [k for k in a if k in b]
    differ = [k for k in both if a[k] != b[k]]
    print(f"{len(a)} kernels in A, {len(b)} in B, {len(both)} in both, {len(differ)} of those differ\n")
    print("| kernel | " + " | ".join(SHORT) + " |\n|" + "---|" * (len(SHORT) + 1))
    for k in both if "--all" in sys.argv else differ:
        print(f"| `{k}` | " + " | ".join(str(x) if x == y else f"{x} -> {y}" for x, y in zip(a[k], b[k])) + " |")
    for tag, one, other in (("A", a, b), ("B", b, a)):
        only = [k for k in one if k not in other]
        if only:
            print(f"\nonly in {tag} ({len(only)}): " + ", ".join(f"`{k}`" for k in only))


if __name__ == "__main__":
    main()
