"""What fused.rasterize(antialiased=True) costs next to the classic frame, at workloads D and B.

    python scripts/antialias_cost.py [--workloads D B] [--rounds 6] [--reps 10] [--out profiles/r11/antialias_cost.json]

One process: per workload the scene once, a spin-up, then `--rounds` alternating blocks (classic, antialiased) of
`--reps` iterations each of
  forward    the per-Gaussian forward's entry point (gs_preprocess_forward_mode, booked as gs_preprocess_forward: k_cull_count,
             k_scan_counts and k_preprocess -- only the last differs between the modes), events around the C-ABI call
             (gaussian_splatting_amd._hip.enable_timing)
  backward   gs_preprocess_backward_mode, booked as gs_preprocess_backward (k_preprocess_bwd alone) on one fixed random slab
  frame      fused.rasterize + image.backward() through the default (native) orchestration, events around the pair
The record holds the median and minimum per mode over all blocks, the per-round medians, the spread of the classic
blocks (max - min of their per-round medians) and antialiased - classic next to it: the mode adds no memory traffic, so
a difference inside that spread is no difference.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("classic", "antialiased")
ENTRY = {"gs_preprocess_forward": "forward", "gs_preprocess_backward": "backward"}   # the labels both modes book under


def measure(workload, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    names = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")

    def stage(aa):
        return fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H,
                                        d["near_thresh"], d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None,
                                        _hip.GS_SORT_PREFIX, antialiased=aa)

    f = {m: stage(m == "antialiased") for m in MODES}
    V = f["classic"].V
    slab = torch.randn(max(V, 1), 9, generator=torch.Generator().manual_seed(3)).to(dev)

    def stage_pass(mode):
        aa = mode == "antialiased"
        stage(aa)
        fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f[mode], slab, antialiased=aa)

    def frame_pass(mode):
        for k in names:
            if getattr(g, k) is not None:
                getattr(g, k).grad = None
        image, _, _ = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg,
                                      antialiased=mode == "antialiased", **d)
        image.backward(gi)

    for m in MODES:
        for _ in range(3):
            stage_pass(m)
    torch.cuda.synchronize()
    _hip.reserve_events(2 * 16 * reps)
    pooled = {m: {"forward": [], "backward": [], "frame": []} for m in MODES}
    per_round = []
    for _ in range(rounds):
        row = {m: {} for m in MODES}
        for m in MODES:
            _hip.enable_timing(True)
            for _ in range(reps):
                stage_pass(m)
            for entry, ms in _hip.collect_timing().items():
                if entry in ENTRY:   # (this block ran mode m only)
                    what = ENTRY[entry]
                    row[m][what] = round(statistics.median(ms), 4)
                    pooled[m][what].extend(ms)
            _hip.enable_timing(False)
        per_round.append(row)
    # whole frames, with gradients
    for k in names:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    for m in MODES:
        for _ in range(3):
            frame_pass(m)
    torch.cuda.synchronize()
    for r in range(rounds):
        for m in MODES:
            pairs = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                frame_pass(m)
                b.record()
                pairs.append((a, b))
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in pairs]
            per_round[r][m]["frame"] = round(statistics.median(ms), 4)
            pooled[m]["frame"].extend(ms)
    out = dict(workload=workload, N=N, W=W, H=H, sh_degree=deg, V=V, S=f["classic"].S,
               median_ms={m: {k: round(statistics.median(v), 4) for k, v in pooled[m].items()} for m in MODES},
               min_ms={m: {k: round(min(v), 4) for k, v in pooled[m].items()} for m in MODES},
               per_round_median_ms=per_round)
    out["classic_spread_ms"] = {k: round(max(r["classic"][k] for r in per_round) - min(r["classic"][k] for r in per_round), 4)
                                for k in ("forward", "backward", "frame")}
    out["antialiased_minus_classic_ms"] = {k: round(out["median_ms"]["antialiased"][k] - out["median_ms"]["classic"][k], 4)
                                           for k in ("forward", "backward", "frame")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["D", "B"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "antialias_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the per-Gaussian entry points and around fused.rasterize + backward, alternating "
                      "classic / antialiased blocks of one process after a spin-up; ms",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.rounds, args.reps)
        print(json.dumps({w: {k: record["workloads"][w][k] for k in ("median_ms", "classic_spread_ms",
                                                                     "antialiased_minus_classic_ms")}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
