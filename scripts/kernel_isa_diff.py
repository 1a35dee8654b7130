#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files: the proof a restructuring leaves the machine code alone.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S render.hip -o before.s      (on the parent)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S render.hip -o after.s       (on the branch)
    scripts/kernel_isa_diff.py before.s after.s

Per kernel: the function body (its label to .Lfunc_end), the .amdhsa_kernel descriptor block and the resource
counts (.set <kernel>.num_vgpr ...), with only the
function index of local labels (.LBB<n>_, .Lfunc_end<n>) normalised -- it shifts when a kernel is added to or
removed from the file.  Prints one line per kernel (instruction count and "identical", "only in ..." or the
unified diff) and exits 1 if a kernel present in both files differs."""
import difflib
import re
import subprocess
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")


def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.startswith("\t.amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = lines.index("\t.amdhsa_kernel " + name)
        d1 = lines.index("\t.end_amdhsa_kernel", d0)
        sets = [l for l in lines[d1:] if l.startswith("\t.set " + name + ".")]   # the resource counts
        text = [LABEL.sub(r".\1N", l) for l in lines[start:end + 1] + lines[d0:d1 + 1] + sets]
        n_instr = sum(1 for l in lines[start:end] if l.startswith("\t") and not l.lstrip().startswith((".", ";")))
        out[name] = (text, n_instr)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        short = [re.sub(r"\(.*", "", s).replace("void ", "") for s in r.stdout.split("\n")]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = list(before) + [n for n in after if n not in before]
    pretty = demangle(names)
    differ = 0
    for n in names:
        if n not in after:
            print(f"{pretty[n]:44s} {before[n][1]:6d} instructions   only in {sys.argv[1]}")
        elif n not in before:
            print(f"{pretty[n]:44s} {after[n][1]:6d} instructions   only in {sys.argv[2]}")
        elif before[n][0] == after[n][0]:
            print(f"{pretty[n]:44s} {after[n][1]:6d} instructions   identical")
        else:
            differ += 1
            print(f"{pretty[n]:44s} {before[n][1]:6d} -> {after[n][1]:6d} instructions   DIFFERENT")
            print("\n".join(difflib.unified_diff(before[n][0], after[n][0], "before", "after", lineterm="", n=2)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
