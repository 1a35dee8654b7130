#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files: the proof a restructuring leaves the machine code alone.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S render.hip -o before.s      (on the parent)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S render.hip -o after.s       (on the branch)
    scripts/kernel_isa_diff.py before.s after.s

Per kernel: the function body (its label to .Lfunc_end), the .amdhsa_kernel descriptor block and the resource
counts (.set <kernel>.num_vgpr ...), with only the
function index of local labels (.LBB<n>_, .Lfunc_end<n>, and BB<n>_ in the loop comments) normalised -- it shifts when a kernel is added to or
removed from the file.  Prints one line per kernel (instruction count and "identical", "only in ..." or the
unified diff) and exits 1 if a kernel present in both files differs.

    scripts/kernel_isa_diff.py --mnemonics before.s after.s

For a kernel whose registers moved but whose instruction stream should not have: compares opcode names only (operands,
register numbers, labels and directives dropped).  Per kernel that differs, instead of the unified diff: the stretches
where the two mnemonic sequences differ, the common tail (from which instruction on each side they are equal to the
end) and the position of the first s_flbit_i32_b64 on each side (the render backward's visit loop opens with it)."""
import difflib
import re
import subprocess
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")
LOOP_NOTE = re.compile(r"\bBB\d+_")   # the same index in the "; in Loop: Header=BB<n>_<m>" comments
LABEL_PAD = re.compile(r"^(\.LBBN_\d+):\s+;")
# (the blanks between a label and its comment: the comment's column is fixed, so they change when the index gains a digit)


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
        text = [LABEL_PAD.sub(r"\1: ;", LOOP_NOTE.sub("BBN_", LABEL.sub(r".\1N", l)))
                for l in lines[start:end + 1] + lines[d0:d1 + 1] + sets]
        mnem = [l.split()[0] for l in lines[start:end] if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
        out[name] = (text, len(mnem), mnem)
    return out


def mnemonic_report(a, b):
    """Lines describing where two mnemonic sequences differ (0-based instruction positions)."""
    first = [seq.index("s_flbit_i32_b64") if "s_flbit_i32_b64" in seq else None for seq in (a, b)]
    out = [f"    first s_flbit_i32_b64: before {first[0]}, after {first[1]}"]
    tail = 0
    while tail < min(len(a), len(b)) and a[-1 - tail] == b[-1 - tail]:
        tail += 1
    out.append(f"    equal from before {len(a) - tail} / after {len(b) - tail} to the end ({tail} mnemonics)")
    for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag != "equal":
            out.append(f"    {tag:8s} before [{i0}, {i1}) {' '.join(a[i0:i1])}  |  after [{j0}, {j1}) {' '.join(b[j0:j1])}")
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        short = [re.sub(r"\(.*", "", s).replace("void ", "") for s in r.stdout.split("\n")]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    mnemonics = "--mnemonics" in sys.argv
    paths = [a for a in sys.argv[1:] if a != "--mnemonics"]
    before, after = kernels(paths[0]), kernels(paths[1])
    names = list(before) + [n for n in after if n not in before]
    pretty = demangle(names)
    differ = 0
    for n in names:
        if n not in after:
            print(f"{pretty[n]:44s} {before[n][1]:6d} instructions   only in {paths[0]}")
        elif n not in before:
            print(f"{pretty[n]:44s} {after[n][1]:6d} instructions   only in {paths[1]}")
        elif before[n][0] == after[n][0]:
            print(f"{pretty[n]:44s} {after[n][1]:6d} instructions   identical")
        else:
            differ += 1
            print(f"{pretty[n]:44s} {before[n][1]:6d} -> {after[n][1]:6d} instructions   DIFFERENT")
            if mnemonics:
                print("\n".join(mnemonic_report(before[n][2], after[n][2])))
            else:
                print("\n".join(difflib.unified_diff(before[n][0], after[n][0], "before", "after", lineterm="", n=2)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
