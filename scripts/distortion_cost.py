"""What the depth-distortion kernels (gs_render_distortion, gs_render_distortion_backward) cost next to the depth kernels
of the same frame (gs_render_zalpha, gs_render_zalpha_backward), which they replace in fused.rasterize_distortion, at
workloads B and D.

    python scripts/distortion_cost.py [--workloads B D] [--rounds 6] [--reps 10] [--out profiles/r14/distortion_cost.json]

One process per run: the per-Gaussian stage, binning, prefix sort and the colour forward (for num_splats_per_pixel)
once per workload, then `--rounds` alternating blocks of `--reps` calls each, on the same lists, events around every
call:

    zalpha_forward        gs_render_zalpha               (k_render_zalpha_fwd)
    distortion_forward    gs_render_distortion           (k_render_distortion_fwd: the same walk, three sums)
    zalpha_backward       gs_render_zalpha_backward      (k_render_zalpha_bwd) into a cleared slab, g_depth and g_alpha
    distortion_backward   gs_render_distortion_backward  (k_render_distortion_bwd) into a cleared slab, all three gradients
    distortion_backward_no_g_dist   the same with grad_distortion NULL: the depth backward's result from the new kernel

The two depth kernels are the yardstick: nothing in the change that added the distortion touches them (their ISA is
identical, profiles/r14/distortion_isa.txt).  The allowance is the 1.5x DESIGN.md 7c gave plain walks.  The record holds
the median and the minimum per block over all rounds, the per-round medians (the spread) and the ratios.  The
prologue that clears the slab is in no figure.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("zalpha_forward", "distortion_forward", "zalpha_backward", "distortion_backward",
          "distortion_backward_no_g_dist")
ALLOWANCE = 1.5


def frame(workload):
    """the workload's frame up to its sorted lists and splat counts -> {block: closure}, (slab, g_z), info"""
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    gx, gd, ga = (gi[..., i].contiguous() for i in range(3))
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, _hip.GS_SORT_PREFIX)
    V = f.V
    rgb_v, xyz_cam = f.rgb_render[:V], f.xyz_cam[:V]
    image, nsp, fw, cost, seg = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                     _hip.GS_SORT_PREFIX, segments=False)
    dep_z, alp_z, t_z = fused.zalpha_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W)
    (dep, dist), alp, t_end = fused.distortion_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W)
    same = bool(torch.equal(dep, dep_z) and torch.equal(alp, alp_z) and torch.equal(t_end, t_z))
    slab = torch.zeros(max(V, 1), fused.SLAB_WIDTH, device=dev)
    g_z = torch.zeros(max(V, 1), device=dev)
    lists = (f.packed, xyz_cam, f.ranges, f.sorted_g, nsp)
    blocks = dict(
        zalpha_forward=lambda: fused.zalpha_forward(*lists, H, W),
        distortion_forward=lambda: fused.distortion_forward(*lists, H, W),
        zalpha_backward=lambda: fused.zalpha_backward(*lists, t_end, gd, ga, H, W, slab, g_z),
        distortion_backward=lambda: fused.distortion_backward(*lists, t_end, dep, alp, gx, gd, ga, H, W, slab, g_z),
        distortion_backward_no_g_dist=lambda: fused.distortion_backward(*lists, t_end, dep, alp, None, gd, ga, H, W,
                                                                        slab, g_z))
    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1),
                walked_entries=int(nsp.sum()), mean_num_splats=round(float(nsp.float().mean()), 1),
                depth_alpha_transmittance_bit_equal=same, distortion_mean=float(dist.mean()),
                distortion_min=float(dist.min()))
    return blocks, (slab, g_z), info


def measure(workload, rounds, reps):
    import torch
    blocks, (slab, g_z), info = frame(workload)
    for _ in range(3):
        for name in BLOCKS:
            blocks[name]()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    per_round, pooled = [], {name: [] for name in BLOCKS}
    for _ in range(rounds):
        row = {}
        for name in BLOCKS:
            if "backward" in name:
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
    ratio_f = round(med["distortion_forward"] / med["zalpha_forward"], 3)
    ratio_b = round(med["distortion_backward"] / med["zalpha_backward"], 3)
    return dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round, ratio_forward=ratio_f,
                ratio_backward=ratio_b,
                ratio_backward_no_g_dist=round(med["distortion_backward_no_g_dist"] / med["zalpha_backward"], 3),
                allowance=ALLOWANCE, forward_within_allowance=ratio_f <= ALLOWANCE,
                backward_within_allowance=ratio_b <= ALLOWANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["B", "D"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "distortion_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the calls, alternating blocks of one process; ratios = gs_render_distortion / "
                      "gs_render_distortion_backward over gs_render_zalpha / gs_render_zalpha_backward of the same "
                      "frame's lists",
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
