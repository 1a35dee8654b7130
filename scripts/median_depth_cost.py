"""What the median-depth kernels (gs_render_median_depth, gs_median_depth_backward) cost at workloads B and D.

    python scripts/median_depth_cost.py [--workloads B D] [--rounds 6] [--reps 10] [--out profiles/r22/median_depth_cost.json]

One process per run: the per-Gaussian stage, binning, prefix sort and the colour forward (for num_splats_per_pixel)
once per workload, then `--rounds` alternating blocks of `--reps` calls each, on the same lists, events around every
call:

    zalpha_forward     gs_render_zalpha          (k_render_zalpha_fwd), which the median forward replaces in the frame
    median_forward     gs_render_median_depth    (k_render_median_fwd: the same walk, two more locals, 8 more bytes out)
    median_backward    gs_median_depth_backward  (k_median_depth_bwd) into a cleared grad_z
    copy_8_bytes       a device copy of 8 bytes per pixel: what the backward reads (index + gradient), moved once
    index_add          the PyTorch composition of the backward: grad_z.index_add_ of the clamped index and the masked
                       gradient (three elementwise launches and the scatter, one atomic per pixel)
    rgbd_frame         fused.rasterize_rgbd forward + backward, a loss on image, depth and alpha
    median_frame       fused.rasterize_median_depth forward + backward, the same loss plus one on median_depth

Yardsticks: the 1.5x DESIGN.md 7c gave a walk variant (median_forward / zalpha_forward) and 1.5x of a copy of its
bytes for the scatter (median_backward / copy_8_bytes).  The record holds the median and the minimum per block over
all rounds, the per-round medians (the spread) and the ratios.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = ("zalpha_forward", "median_forward", "median_backward", "copy_8_bytes", "index_add", "rgbd_frame",
          "median_frame")
ALLOWANCE = 1.5


def frame(workload):
    """the workload's frame up to its sorted lists and splat counts -> {block: closure}, grad_z, info"""
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    gm, gd, ga = (gi[..., i].contiguous() for i in range(3))
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, _hip.GS_SORT_PREFIX)
    V = f.V
    rgb_v, xyz_cam = f.rgb_render[:V], f.xyz_cam[:V]
    image, nsp, fw, cost, seg = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                     _hip.GS_SORT_PREFIX, segments=False)
    dep_z, alp_z, t_z = fused.zalpha_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W)
    (dep, md, mi), alp, t_end = fused.median_depth_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, nsp, H, W)
    same = bool(torch.equal(dep, dep_z) and torch.equal(alp, alp_z) and torch.equal(t_end, t_z))
    has = mi >= 0
    gathered = bool(torch.equal(md[has], xyz_cam[:, 2][mi[has].long()]))
    g_z = torch.zeros(max(V, 1), device=dev)
    fused.median_depth_backward(mi, gm, H, W, g_z)
    by_torch = torch.zeros(max(V, 1), device=dev, dtype=torch.float64)
    by_torch.index_add_(0, mi[has].long(), gm[has].double())
    mag = torch.zeros(max(V, 1), device=dev, dtype=torch.float64).index_add_(0, mi[has].long(), gm[has].double().abs())
    worst = float(((g_z.double() - by_torch).abs() / mag.clamp(min=1e-300))[mag > 0].max())
    counts = torch.bincount(mi[has].long(), minlength=max(V, 1))
    src, dst = torch.randn(H, W, 2, device=dev), torch.empty(H, W, 2, device=dev)
    lists = (f.packed, xyz_cam, f.ranges, f.sorted_g, nsp)
    for k in ("xyz", "quaternion", "scale", "opacity", "rgb"):
        getattr(g, k).requires_grad_(True)
    kw = dict(use_sh_precompute=True, background_rgb=bg, **DEFAULTS)

    def rgbd_frame():
        image, depth, alpha, mask, uv = fused.rasterize_rgbd(g, T, cam, **kw)
        torch.autograd.backward([image, depth, alpha], [gi, gd, ga])

    def median_frame():
        image, depth, alpha, median, index, mask, uv = fused.rasterize_median_depth(g, T, cam, **kw)
        torch.autograd.backward([image, depth, alpha, median], [gi, gd, ga, gm])

    blocks = dict(
        zalpha_forward=lambda: fused.zalpha_forward(*lists, H, W),
        median_forward=lambda: fused.median_depth_forward(*lists, H, W),
        median_backward=lambda: fused.median_depth_backward(mi, gm, H, W, g_z),
        copy_8_bytes=lambda: dst.copy_(src),
        index_add=lambda: g_z.index_add_(0, mi.clamp(min=0).long().view(-1),
                                         torch.where(mi >= 0, gm, torch.zeros_like(gm)).view(-1)),
        rgbd_frame=rgbd_frame, median_frame=median_frame)
    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1),
                mean_num_splats=round(float(nsp.float().mean()), 1), depth_alpha_transmittance_bit_equal=same,
                median_depth_is_z_of_index=gathered, pixels_without_contributor=float((~has).float().mean()),
                pixels_crossed=float((alp >= 0.5).float().mean()), selected_gaussians=int((counts > 0).sum()),
                most_pixels_on_one_gaussian=int(counts.max()), backward_noise_vs_float64=worst)
    return blocks, g_z, info


def measure(workload, rounds, reps):
    import torch
    blocks, g_z, info = frame(workload)
    for _ in range(3):
        for name in BLOCKS:
            blocks[name]()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    per_round, pooled = [], {name: [] for name in BLOCKS}
    for _ in range(rounds):
        row = {}
        for name in BLOCKS:
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
    ratio_f = round(med["median_forward"] / med["zalpha_forward"], 3)
    ratio_b = round(med["median_backward"] / med["copy_8_bytes"], 3)
    return dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round, ratio_forward=ratio_f,
                ratio_backward_over_copy=ratio_b,
                ratio_backward_over_index_add=round(med["median_backward"] / med["index_add"], 3),
                ratio_frame=round(med["median_frame"] / med["rgbd_frame"], 3),
                allowance=ALLOWANCE, forward_within_allowance=ratio_f <= ALLOWANCE,
                backward_within_allowance=ratio_b <= ALLOWANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["B", "D"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "median_depth_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the calls, alternating blocks of one process; ratio_forward = gs_render_median_depth "
                      "/ gs_render_zalpha on the same frame's lists, ratio_backward_over_copy = gs_median_depth_backward "
                      "/ a device copy of its 8 bytes per pixel, ratio_frame = rasterize_median_depth / rasterize_rgbd, "
                      "forward + backward",
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
