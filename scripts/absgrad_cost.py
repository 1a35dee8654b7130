"""What the absgrad form of the colour backward (gs_render_tiles_backward_slab_abs, k_render_bwd_abs) costs next to the
plain one (gs_render_tiles_backward_slab, k_render_bwd<float, 1>) on the same frame, at bench.py's workloads D and B.

    python scripts/absgrad_cost.py [--workloads D B] [--rounds 6] [--reps 10] [--out profiles/r16/absgrad_cost.json]

One process per run: the per-Gaussian stage, binning, prefix sort, the colour forward and the backward's prologue
(the tile order) once per workload, then `--rounds` alternating blocks of `--reps` calls each, on the same lists,
events around every call:

    plain_a    gs_render_tiles_backward_slab      into a cleared slab, tile_order given
    absgrad    gs_render_tiles_backward_slab_abs  into a cleared slab and a cleared [V, 2], the same tile_order
    plain_b    the plain call once more

The plain kernel is the yardstick and the parent's own: its ISA is identical to the parent commit's
(profiles/r16/absgrad_isa.txt).  plain_a against plain_b, per round, is the spread of that unchanged kernel between
its own blocks -- what a ratio has to exceed to mean anything.  The allowance for a walk variant is the 1.5x of
DESIGN.md 7c to 7g.  The record holds the median and the minimum per block over all rounds, the per-round medians and
the ratios.  Clearing the slab and the prologue are in no figure.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("plain_a", "absgrad", "plain_b")
ALLOWANCE = 1.5


def frame(workload):
    """the workload's frame up to the forward's outputs and the tile order -> {block: closure}, buffers, info"""
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, _hip.GS_SORT_PREFIX)
    V = f.V
    rgb_v = f.rgb_render[:V]
    image, nsp, fw, cost, seg = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                     _hip.GS_SORT_PREFIX, segments=False)
    nty = (H + 15) // 16
    slab = torch.zeros(max(V, 1), fused.SLAB_WIDTH, device=dev)
    uv_abs = torch.zeros(max(V, 1), 2, device=dev)
    order = torch.empty(cost.numel() + 8, dtype=torch.int32, device=dev)
    p, stream = _hip.ptr, _hip.current_stream
    _hip.call("gs_render_backward_prologue", None, 0, p(cost), p(order), W, H, 0, nty, stream())
    walk = (p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp), p(fw), p(gi), W, H, 0, nty, p(slab), 0, None,
            p(order), None, None, None, None, _hip.GS_BACKWARD_DEFAULT)
    plain = lambda: _hip.call("gs_render_tiles_backward_slab", *walk, stream())
    blocks = dict(plain_a=plain, plain_b=plain,
                  absgrad=lambda: _hip.call("gs_render_tiles_backward_slab_abs", *walk, None, p(uv_abs), stream()))
    # one call of each into cleared buffers: the nine sums agree, and what the new signal is next to the old
    plain()
    ref = slab.clone()
    slab.zero_()
    blocks["absgrad"]()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    signed = slab[:V, fused.SLAB_UV].abs()
    seen = signed.sum(dim=1) > 0
    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1),
                walked_entries=int(nsp.sum()),
                slab_max_diff_over_max=float((slab - ref).abs().max()) / max(scale, 1e-30),
                median_absgrad_over_signed=float((uv_abs[:V][seen].sum(dim=1) / signed[seen].sum(dim=1)).median()),
                absgrad_below_signed_rows=int((uv_abs[:V] * (1 + 1e-4) + 1e-30 < signed).any(dim=1).sum()))
    return blocks, (slab, uv_abs), info


def measure(workload, rounds, reps):
    import torch
    blocks, buffers, info = frame(workload)
    for _ in range(3):
        for name in BLOCKS:
            blocks[name]()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    per_round, pooled = [], {name: [] for name in BLOCKS}
    for _ in range(rounds):
        row = {}
        for name in BLOCKS:
            for b in buffers:
                b.zero_()
            for a, b in events:
                a.record()
                blocks[name]()
                b.record()
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in events]
            row[name] = round(statistics.median(ms), 4)
            pooled[name].extend(ms)
        per_round.append(row)
    med = {k: round(statistics.median(v), 4) for k, v in pooled.items()}
    mn = {k: round(min(v), 4) for k, v in pooled.items()}
    plain = statistics.median(pooled["plain_a"] + pooled["plain_b"])
    spread = [round(r["plain_b"] / r["plain_a"], 4) for r in per_round]
    ratio = round(med["absgrad"] / plain, 3)
    return dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round, plain_median_ms=round(plain, 4),
                ratio_absgrad_over_plain=ratio, ratio_of_minima=round(mn["absgrad"] / min(mn["plain_a"], mn["plain_b"]), 3),
                plain_block_to_block=spread, plain_block_to_block_max_dev=round(max(abs(s - 1) for s in spread), 4),
                allowance=ALLOWANCE, within_allowance=ratio <= ALLOWANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["D", "B"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "absgrad_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the calls, alternating blocks of one process; ratio = "
                      "gs_render_tiles_backward_slab_abs over gs_render_tiles_backward_slab on the same frame's lists; "
                      "plain_block_to_block = the unchanged kernel's second block over its first, per round",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.rounds, args.reps)
        print(json.dumps({w: {k: v for k, v in record["workloads"][w].items()
                              if k == "median_ms" or k.startswith("ratio") or k.startswith("plain_block")}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
