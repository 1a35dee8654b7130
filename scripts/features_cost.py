"""What the feature-map kernels (gs_render_features, gs_render_features_backward) cost at C = 1, 4, 16, 32 next to the
colour and the depth / alpha kernels of the same frame, at workloads B and D.

    python scripts/features_cost.py [--workloads B D] [--channels 1 4 16 32] [--rounds 6] [--reps 10]
                                    [--out profiles/r09/features_cost.json]

One process per run, as scripts/rgbd_cost.py: the per-Gaussian stage, binning and prefix sort once per workload, then
`--rounds` alternating blocks of `--reps` x (colour forward, colour backward), `--reps` x (depth forward, prologue +
depth backward) and, per channel count, `--reps` x (features forward, prologue + features backward with
grad_features; at C = 4 also without) on the same lists, events around every C-ABI call (gaussian_splatting_amd._hip.enable_timing).  The
record holds the median and the minimum per entry point (the features' per channel count) over all blocks, the
per-round medians (the spread) and the ratios features / depth and features / colour.  The yardstick of the one
expectation stated in advance (C = 4 within 1.5x of the depth kernels) is the depth kernels, which this work left alone.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLOUR_FWD = ("gs_render_tiles_prefix", "gs_render_tiles_packed")


def frame(workload, channels):
    """the workload's frame up to its sorted lists, and closures for the passes"""
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
    rgb_v, xyz_cam = f.rgb_render[:V], f.xyz_cam[:V]
    gen = torch.Generator().manual_seed(2)
    feats = {C: torch.randn(V, C, generator=gen).to(dev) for C in channels}
    g_maps = {C: (torch.randn(H, W, C, generator=gen) / (W * H)).to(dev) for C in channels}
    state = {}

    def colour():
        image, nsp, fw, cost, seg = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                         _hip.GS_SORT_PREFIX, segments=False)
        state.update(nsp=nsp)
        return fused.render_backward(f.packed, rgb_v, f.ranges, f.sorted_g, bg, nsp, fw, gi, H, W, None, V, cost)

    def depth():
        dep, alp, t_end = fused.zalpha_forward(f.packed, xyz_cam, f.ranges, f.sorted_g, state["nsp"], H, W)
        slab, g_z = fused.render_backward(f.packed, rgb_v, f.ranges, f.sorted_g, bg, state["nsp"], None, None, H, W, None,
                                          V, tail=max(V, 1))
        fused.zalpha_backward(f.packed, xyz_cam, f.ranges, f.sorted_g, state["nsp"], t_end, gd, ga, H, W, slab, g_z)
        return dep, slab, g_z

    def features(C, with_grad_features=True):
        def run():
            fmap, alp, t_end = fused.features_forward(f.packed, feats[C], f.ranges, f.sorted_g, state["nsp"], H, W)
            slab = fused.render_backward(f.packed, rgb_v, f.ranges, f.sorted_g, bg, state["nsp"], None, None, H, W, None, V)
            g_feat = torch.zeros_like(feats[C]) if with_grad_features else None
            fused.features_backward(f.packed, feats[C], f.ranges, f.sorted_g, state["nsp"], t_end, g_maps[C], ga, H, W,
                                    slab, g_feat)
            return fmap, slab, g_feat
        return run

    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1))
    runs = {f"[C={C}]": features(C) for C in channels}
    # the same walk without the feature-gradient contraction (grad_features NULL): what the geometry part alone costs
    runs.update({f"[C={C}, no grad_features]": features(C, False) for C in channels if C == 4})
    return colour, depth, runs, state, info


def measure(workload, channels, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip
    colour, depth, features, state, info = frame(workload, channels)
    blocks = [("", colour), ("", depth)] + list(features.items())
    for _ in range(3):
        for _, block in blocks:
            block()
    torch.cuda.synchronize()
    info["mean_num_splats"] = round(float(state["nsp"].float().mean()), 1)
    _hip.reserve_events(2 * 8 * reps)
    per_round, pooled = [], {}
    for _ in range(rounds):
        row = {}
        for tag, block in blocks:
            _hip.enable_timing(True)
            for _ in range(reps):
                block()
            for name, ms in _hip.collect_timing().items():
                key = name + tag if name.startswith("gs_render_features") else name
                if tag and key == name:
                    continue   # (the shared prologue of a features block: counted with the depth block's)
                row[key] = round(statistics.median(ms), 4)
                pooled.setdefault(key, []).extend(ms)
            _hip.enable_timing(False)
        per_round.append(row)
    med = {k: round(statistics.median(v), 4) for k, v in sorted(pooled.items())}
    mn = {k: round(min(v), 4) for k, v in sorted(pooled.items())}
    fwd_colour = sum(med.get(k, 0.0) for k in COLOUR_FWD)
    ratios = {}
    for C in channels:
        fw, bw = med[f"gs_render_features[C={C}]"], med[f"gs_render_features_backward[C={C}]"]
        ratios[f"C={C}"] = dict(forward_over_depth=round(fw / med["gs_render_zalpha"], 3),
                                backward_over_depth=round(bw / med["gs_render_zalpha_backward"], 3),
                                forward_over_colour=round(fw / fwd_colour, 3),
                                backward_over_colour=round(bw / med["gs_render_tiles_backward_slab"], 3))
    return dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round, ratios=ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["B", "D"])
    ap.add_argument("--channels", nargs="+", type=int, default=[1, 4, 16, 32])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "features_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the C-ABI entry points, alternating blocks of one process; features forward = "
                      "gs_render_features, backward = gs_render_features_backward with grad_features (both without the "
                      "shared prologue); ratios over the depth kernels (gs_render_zalpha / _backward) and over the colour "
                      "kernels of the same lists",
              "rounds": args.rounds, "reps": args.reps, "channels": args.channels, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.channels, args.rounds, args.reps)
        print(json.dumps({w: {k: record["workloads"][w][k] for k in ("median_ms", "ratios")}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
