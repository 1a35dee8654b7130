"""What the selective optimizer step (gs_adam_step_rows, k_adam_rows) costs next to the dense one (gs_adam_step, k_adam)
on the six parameter tensors of workload D's size, by how much of the scene the mask leaves visible.

    python scripts/selective_adam_cost.py [--n 2860000] [--rounds 6] [--reps 10]
                                          [--out profiles/r10/selective_adam_cost.json]

One process, events around every C-ABI call (gaussian_splatting_amd._hip.enable_timing), as scripts/features_cost.py:
`--rounds` rounds, each of which runs, per case, a block of `--reps` dense steps and then a block of `--reps` selective
steps with the case's mask on the same tensors.  Cases: none culled; random masks with 50 / 25 / 10 / 2 % of the rows
visible; one contiguous visible block of the same fractions; all culled.  Per case the record holds the median and
minimum ms over all its blocks, the per-block medians, the ratio to the dense kernel's median in the same record, the
model bytes (28 B per visible element plus one mask byte per row and tensor) and the rate they imply; for the dense
kernel also the spread of its per-block medians, the yardstick of "no slower with nothing culled".
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (3, 4, 3, 1, 3, 45)   # xyz, quaternion, scale, opacity, rgb, sh at degree 3
LRS = (0.0002, 0.004, 0.01, 0.02, 0.004, 0.0002)
FRACTIONS = (0.5, 0.25, 0.1, 0.02)


def masks(n, gen):
    """-> {case: (culled [n] bool on the device, visible rows)}"""
    import torch
    out = {"none_culled": torch.zeros(n, dtype=torch.bool)}
    for f in FRACTIONS:
        out[f"random_{round(100 * f)}pc_visible"] = torch.rand(n, generator=gen) >= f
    for f in FRACTIONS:
        m = torch.ones(n, dtype=torch.bool)
        a = int(0.37 * n)
        m[a:a + int(f * n)] = False
        out[f"block_{round(100 * f)}pc_visible"] = m
    out["all_culled"] = torch.ones(n, dtype=torch.bool)
    return {k: (m.cuda(), int((~m).sum())) for k, m in out.items()}


def measure(n, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip
    gen = torch.Generator().manual_seed(0)
    dev = torch.device("cuda", 0)
    p = [torch.randn(n, w, device=dev) for w in WIDTHS]
    g = [1e-3 * torch.randn(n, w, device=dev) for w in WIDTHS]
    m = [torch.zeros(n, w, device=dev) for w in WIDTHS]
    v = [torch.zeros(n, w, device=dev) for w in WIDTHS]
    k = len(WIDTHS)
    ptrs = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
    numel = (ctypes.c_int64 * k)(*[t.numel() for t in p])
    width = (ctypes.c_int64 * k)(*WIDTHS)
    lr, step = (ctypes.c_double * k)(*LRS), (ctypes.c_int64 * k)(*([100] * k))
    stream = _hip.current_stream()
    cases = masks(n, gen)

    def dense():
        _hip.call("gs_adam_step", k, ptrs(p), ptrs(g), ptrs(m), ptrs(v), numel, lr, step, 0.9, 0.999, 1e-15, stream)

    def rows(mask):
        _hip.call("gs_adam_step_rows", k, ptrs(p), ptrs(g), ptrs(m), ptrs(v), numel, width, mask.data_ptr(), n, lr, step,
                  0.9, 0.999, 1e-15, stream)

    def block(fn, name):
        _hip.enable_timing(True)
        for _ in range(reps):
            fn()
        ms = _hip.collect_timing()[name]
        _hip.enable_timing(False)
        return ms

    for _ in range(3):
        dense()
        for mask, _ in cases.values():
            rows(mask)
    torch.cuda.synchronize()
    _hip.reserve_events(2 * reps)
    dense_blocks, case_blocks = [], {c: [] for c in cases}
    for _ in range(rounds):
        for c, (mask, _) in cases.items():
            dense_blocks.append(block(dense, "gs_adam_step"))
            case_blocks[c].append(block(lambda: rows(mask), "gs_adam_step_rows"))

    def summary(blocks):
        pooled = [x for b in blocks for x in b]
        return dict(median_ms=round(statistics.median(pooled), 4), min_ms=round(min(pooled), 4),
                    block_median_ms=[round(statistics.median(b), 4) for b in blocks])

    elements = sum(WIDTHS) * n
    d = summary(dense_blocks)
    d["model_bytes"] = 28 * elements
    d["model_gbs"] = round(d["model_bytes"] / d["median_ms"] / 1e6, 1)
    lo, hi = min(d["block_median_ms"]), max(d["block_median_ms"])
    d["block_spread"] = dict(min_ms=lo, max_ms=hi, max_over_median=round(hi / d["median_ms"], 4),
                             min_over_median=round(lo / d["median_ms"], 4))
    out = {}
    for c, (mask, visible) in cases.items():
        s = summary(case_blocks[c])
        s["visible_rows"], s["visible_fraction"] = visible, round(visible / n, 4)
        s["ratio_to_dense"] = round(s["median_ms"] / d["median_ms"], 4)
        s["model_bytes"] = 28 * sum(WIDTHS) * visible + len(WIDTHS) * n
        s["model_gbs"] = round(s["model_bytes"] / s["median_ms"] / 1e6, 1)
        out[c] = s
    return dict(N=n, elements=elements, gs_adam_step=d, gs_adam_step_rows=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_860_000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "selective_adam_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the C-ABI entry points, one process; per round and case a block of dense steps "
                      "(gs_adam_step) then a block of selective steps (gs_adam_step_rows) with the case's mask, on the same "
                      "six fp32 tensors of widths 3, 4, 3, 1, 3, 45; model bytes = 28 B per stepped element + 1 mask byte "
                      "per row and tensor; ratio_to_dense = median over the dense kernel's median of this record",
              "rounds": args.rounds, "reps": args.reps}
    record.update(measure(args.n, args.rounds, args.reps))
    print(json.dumps({"gs_adam_step": {k: record["gs_adam_step"][k] for k in ("median_ms", "block_spread")}}))
    for c, s in record["gs_adam_step_rows"].items():
        print(json.dumps({c: {k: s[k] for k in ("median_ms", "ratio_to_dense", "model_gbs")}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(os.path.abspath(args.out), ROOT)}))


if __name__ == "__main__":
    main()
