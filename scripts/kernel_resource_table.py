"""Kernel resource tables of two builds of one translation unit, side by side.

    hipcc <the Makefile's FLAGS> -Rpass-analysis=kernel-resource-usage -c preprocess.hip -o /dev/null 2> base.log
    ... (the other tree) ...                                                                       2> new.log
    python scripts/kernel_resource_table.py base.log new.log [--drop-trailing-false N] > table.md

Reads the compiler's remarks (SGPRs, VGPRs, scratch, occupancy, LDS per kernel), demangles the names with c++filt and
prints (1) every kernel present on both sides with whether the five numbers are equal, (2) the kernels of the second
log alone.  --drop-trailing-false N: a kernel of the second log whose template list ends in up to N `false` arguments
that the first log's kernels do not have (a template flag added with a default) is matched to the name without them.
"""
import argparse
import re
import subprocess
import sys

FIELDS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS"))


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and name is not None:
            out[name][m.group(1).strip()] = m.group(2)
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for mangled, full in zip(names, plain):
        short = re.sub(r"^void ", "", full)
        depth, cut = 0, len(short)
        for i, ch in enumerate(short):   # the argument list: the first '(' outside the template brackets
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        res[short[:cut].replace("gs::", "")] = tuple(out[mangled].get(k, "?") for k, _ in FIELDS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--drop-trailing-false", type=int, default=0)
    a = ap.parse_args()
    base, new = parse(a.base), parse(a.new)
    matched, only_new = [], []
    for name, vals in new.items():
        key = name
        for _ in range(a.drop_trailing_false + 1):
            if key in base:
                break
            key = re.sub(r", false>$", ">", key)
        if key in base:
            matched.append((key, base[key], vals))
        else:
            only_new.append((name, vals))
    missing = sorted(set(base) - {k for k, _, _ in matched})
    head = " | ".join(short for _, short in FIELDS)
    print(f"## kernels of both builds ({len(matched)}; {sum(b == n for _, b, n in matched)} equal)\n")
    print(f"| kernel | {head} | equal |\n|---|" + "---|" * (len(FIELDS) + 1))
    for key, b, n in sorted(matched):
        cells = " | ".join(x if x == y else f"{x} -> {y}" for x, y in zip(b, n))
        print(f"| `{key}` | {cells} | {'yes' if b == n else 'NO'} |")
    print(f"\n## kernels of the second build alone ({len(only_new)})\n")
    print(f"| kernel | {head} |\n|---|" + "---|" * len(FIELDS))
    for name, n in sorted(only_new):
        print(f"| `{name}` | " + " | ".join(n) + " |")
    if missing:
        print("\n## kernels of the first build alone\n")
        for k in missing:
            print(f"* `{k}`")
    return 0 if not missing and all(b == n for _, b, n in matched) else 1


if __name__ == "__main__":
    sys.exit(main())
