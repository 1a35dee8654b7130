"""What the contribution-statistics kernel (gs_render_contributions) costs next to the depth kernels of the same frame
(gs_render_zalpha, gs_render_zalpha_backward), at workloads B and D.

    python scripts/contributions_cost.py [--workloads B D] [--rounds 6] [--reps 10] [--out profiles/r13/contributions_cost.json]

One process per run: the per-Gaussian stage, binning, prefix sort and the colour forward (for num_splats_per_pixel)
once per workload, then `--rounds` alternating blocks of `--reps` calls each, on the same lists, events around every
call:

    zalpha_forward        gs_render_zalpha
    zalpha_backward       gs_render_zalpha_backward into a cleared slab (the prologue is not in the figure)
    contributions         gs_render_contributions, three outputs, row_index = the frame's visible indices into [N] arrays
    contributions_max     the same with weight_max alone (weight_sum and pixel_count NULL)
    contributions_chunk256 three outputs with 256 entries staged per step instead of 64 (gs_debug_contributions_chunk)

The two depth kernels are the yardstick: nothing in the change that added the statistics touches them.  The record
holds the median and the minimum per block over all rounds, the per-round medians (the spread) and the ratios of the
contributions kernel to each of the two.  The statistics buffers are cleared once per workload and accumulate over the
calls (the atomics cost the same whatever the rows hold).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("zalpha_forward", "zalpha_backward", "contributions", "contributions_max", "contributions_chunk256")


def frame(workload):
    """the workload's frame up to its sorted lists and splat counts -> {block: closure}, info"""
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    gd, ga = gi[..., 0].contiguous(), gi[..., 1].contiguous()
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, _hip.GS_SORT_PREFIX)
    V = f.V
    rgb_v, xyz_cam, vis_idx = f.rgb_render[:V], f.xyz_cam[:V], f.vis_idx[:V]
    image, nsp, fw, cost, seg = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                     _hip.GS_SORT_PREFIX, segments=False)
    dep, alp, t_end = fused.zalpha_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W)
    slab = torch.zeros(max(V, 1), fused.SLAB_WIDTH, device=dev)
    g_z = torch.zeros(max(V, 1), device=dev)
    stats = fused.ContributionStats.zeros(N, dev)
    lib = _hip.lib()

    def contributions(wsum, wmax, count, chunk=64):
        before = lib.gs_debug_contributions_chunk(chunk)
        try:
            fused.contributions_forward(f.packed, f.ranges, f.sorted_g, nsp, H, W, vis_idx, wsum, wmax, count)
        finally:
            lib.gs_debug_contributions_chunk(before)

    blocks = dict(
        zalpha_forward=lambda: fused.zalpha_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W),
        zalpha_backward=lambda: fused.zalpha_backward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, t_end, gd, ga, H, W,
                                                      slab, g_z),
        contributions=lambda: contributions(stats.weight_sum, stats.weight_max, stats.pixel_count),
        contributions_max=lambda: contributions(None, stats.weight_max, None),
        contributions_chunk256=lambda: contributions(stats.weight_sum, stats.weight_max, stats.pixel_count, 256))
    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1),
                walked_entries=int(nsp.sum()), mean_num_splats=round(float(nsp.float().mean()), 1))
    return blocks, (slab, g_z), stats, info


def measure(workload, rounds, reps):
    import torch
    blocks, (slab, g_z), stats, info = frame(workload)
    for _ in range(3):
        for name in BLOCKS:
            blocks[name]()
    torch.cuda.synchronize()
    info["touched"] = int(stats.touched.sum())     # of the V visible Gaussians, after the warm-up calls
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    per_round, pooled = [], {name: [] for name in BLOCKS}
    for _ in range(rounds):
        row = {}
        for name in BLOCKS:
            if name == "zalpha_backward":
                slab.zero_()
                g_z.zero_()
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
    return dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round,
                ratio_to_zalpha_forward=round(med["contributions"] / med["zalpha_forward"], 3),
                ratio_to_zalpha_backward=round(med["contributions"] / med["zalpha_backward"], 3),
                ratio_max_alone=round(med["contributions_max"] / med["contributions"], 3),
                ratio_chunk256=round(med["contributions_chunk256"] / med["contributions"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["B", "D"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "contributions_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the calls, alternating blocks of one process; ratios = gs_render_contributions (three "
                      "outputs, 64 entries per step) over gs_render_zalpha / gs_render_zalpha_backward of the same "
                      "frame, and the weight_max-only and 256-entry forms over the three-output one",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.rounds, args.reps)
        print(json.dumps({w: {k: v for k, v in record["workloads"][w].items() if k == "median_ms" or k.startswith("ratio")}}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
