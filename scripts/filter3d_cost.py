"""What the 3D smoothing filter costs: rasterize(antialiased=True) with and without filter3d=, and gs_filter3d_rate, at
workloads D and B.

    python scripts/filter3d_cost.py [--workloads D B] [--rounds 6] [--reps 10] [--cameras 200]
                                    [--out profiles/r19/filter3d_cost.json]

One process: per workload the scene once, the filter from the scene's own camera and `--cameras` - 1 more around its
centre (gs_filter3d_rate, variance 0.2), a spin-up, then `--rounds` alternating blocks (antialiased, antialiased +
filter) of `--reps` iterations each of
  forward    the per-Gaussian forward's entry point (gs_preprocess_forward_filtered, booked as gs_preprocess_forward:
             k_cull_count, k_scan_counts and k_preprocess -- only the last differs), events around the C-ABI call
  backward   gs_preprocess_backward_filtered, booked as gs_preprocess_backward (k_preprocess_bwd alone), one fixed slab
  frame      fused.rasterize + image.backward() through the default (native) orchestration, events around the pair
and, in blocks of the same size,
  rate       gs_filter3d_rate over all cameras (one launch)
  torch      the per-camera PyTorch composition of the same result (transform, projection, in-view test, maximum)
  copy       a device copy of 16 bytes per Gaussian (the rate kernel's traffic: xyz in, rate in and out)
The record holds the medians, the per-round medians, the spread of the unfiltered blocks (max - min of their per-round
medians) and filtered - unfiltered next to it: the filter adds 4 bytes to roughly 330 per visible Gaussian.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("antialiased", "filtered")
ENTRY = {"gs_preprocess_forward": "forward", "gs_preprocess_backward": "backward"}   # the labels both modes book under


def cameras_around(T, K, centre, n, dev):
    """T and n - 1 poses looking at `centre` from distances 0.5 .. 2 times the scene camera's -> [n, 4, 4], [n, 3, 3]"""
    import torch
    gen = torch.Generator().manual_seed(5)
    base = float((torch.linalg.inv(T.double().cpu())[:3, 3] - centre).norm())
    Ts = [T.double().cpu()]
    for _ in range(n - 1):
        fwd = torch.randn(3, generator=gen, dtype=torch.float64)
        fwd = fwd / fwd.norm()
        eye = centre - base * (0.5 + 1.5 * float(torch.rand(1, generator=gen))) * fwd
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) if abs(float(fwd[2])) < 0.9 else \
            torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
        right = torch.linalg.cross(fwd, up)
        right = right / right.norm()
        A = torch.stack([right, torch.linalg.cross(fwd, right), fwd])
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = A, -A @ eye
        Ts.append(M)
    return torch.stack(Ts).float().to(dev).contiguous(), K[None].repeat(n, 1, 1).contiguous()


def torch_rate(xyz, Ts, Ks, W, H, near=0.2, pad=0.15):
    """the per-camera PyTorch composition of gs_filter3d_rate (pinhole)"""
    import torch
    rate = torch.zeros(xyz.shape[0], device=xyz.device)
    for k in range(Ts.shape[0]):
        c = xyz @ Ts[k, :3, :3].T + Ts[k, :3, 3]
        z = c[:, 2]
        u = Ks[k, 0, 0] * c[:, 0] / z + Ks[k, 0, 2]
        v = Ks[k, 1, 1] * c[:, 1] / z + Ks[k, 1, 2]
        seen = (z > near) & (u > -pad * W) & (u < W + pad * W) & (v > -pad * H) & (v < H + pad * H)
        rate = torch.where(seen, torch.maximum(rate, torch.maximum(Ks[k, 0, 0], Ks[k, 1, 1]) / z), rate)
    return rate


def timed_blocks(fn, rounds, reps):
    import torch
    out = []
    for _ in range(rounds):
        pairs = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        out.append([a.elapsed_time(b) for a, b in pairs])
    return out


def measure(workload, rounds, reps, n_cameras):
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
    Ts, Ks = cameras_around(T, cam.K, g.xyz.double().mean(dim=0).cpu(), n_cameras, dev)
    rate = fused.filter3d_rate(g.xyz, Ts, Ks, (W, H))
    phi = fused.filter3d_from_rate(rate)
    filt = {"antialiased": None, "filtered": phi}

    def stage(m):
        return fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H,
                                        d["near_thresh"], d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None,
                                        _hip.GS_SORT_PREFIX, antialiased=True, filter3d=filt[m])

    f = {m: stage(m) for m in MODES}
    V = f["antialiased"].V
    slab = torch.randn(max(V, 1), 9, generator=torch.Generator().manual_seed(3)).to(dev)

    def stage_pass(m):
        stage(m)
        fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f[m], slab, antialiased=True, filter3d=filt[m])

    def frame_pass(m):
        for k in names:
            if getattr(g, k) is not None:
                getattr(g, k).grad = None
        image, _, _ = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True,
                                      filter3d=filt[m], **d)
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
                    row[m][ENTRY[entry]] = round(statistics.median(ms), 4)
                    pooled[m][ENTRY[entry]].extend(ms)
            _hip.enable_timing(False)
        per_round.append(row)
    for k in names:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    for m in MODES:
        for _ in range(3):
            frame_pass(m)
    torch.cuda.synchronize()
    for r in range(rounds):
        for m in MODES:
            ms = timed_blocks(lambda: frame_pass(m), 1, reps)[0]
            per_round[r][m]["frame"] = round(statistics.median(ms), 4)
            pooled[m]["frame"].extend(ms)
    keys = ("forward", "backward", "frame")
    out = dict(workload=workload, N=N, W=W, H=H, sh_degree=deg, V=V, S=f["antialiased"].S,
               rows_some_camera_sees=int((rate > 0).sum()),
               median_ms={m: {k: round(statistics.median(v), 4) for k, v in pooled[m].items()} for m in MODES},
               min_ms={m: {k: round(min(v), 4) for k, v in pooled[m].items()} for m in MODES},
               per_round_median_ms=per_round)
    out["unfiltered_spread_ms"] = {k: round(max(r["antialiased"][k] for r in per_round) -
                                            min(r["antialiased"][k] for r in per_round), 4) for k in keys}
    out["filtered_minus_unfiltered_ms"] = {k: round(out["median_ms"]["filtered"][k] - out["median_ms"]["antialiased"][k], 4)
                                           for k in keys}
    out["filtered_minus_unfiltered_percent"] = {k: round(100.0 * out["filtered_minus_unfiltered_ms"][k] /
                                                         out["median_ms"]["antialiased"][k], 2) for k in keys}
    # ---- the rate kernel ----
    with torch.no_grad():
        buf = torch.zeros(N, device=dev)
        src, dst = torch.empty(2 * N, 2, device=dev), torch.empty(2 * N, 2, device=dev)   # 16 B read + 16 B written per two rows
        want = torch_rate(g.xyz, Ts, Ks, W, H)
        got = fused.filter3d_rate(g.xyz, Ts, Ks, (W, H))
        agree = float(((got - want).abs() <= 1e-4 * want.abs()).float().mean())
        sizes = torch.tensor([[W, H]], dtype=torch.int32, device=dev).repeat(n_cameras, 1)
        stream = _hip.current_stream()
        p = _hip.ptr
        run = {"rate": lambda: _hip.call("gs_filter3d_rate", p(g.xyz), p(Ts), p(Ks), p(sizes), n_cameras, N, 0.2, 0.15,
                                         _hip.GS_RASTER_CLASSIC, p(buf), stream),
               "copy": lambda: dst[:N].copy_(src[:N]),
               "torch": lambda: torch_rate(g.xyz, Ts, Ks, W, H)}
        rate_ms = {}
        for name, fn in run.items():
            fn()
            torch.cuda.synchronize()
            blocks = timed_blocks(fn, rounds if name != "torch" else 2, reps if name != "torch" else 3)
            rate_ms[name] = dict(median_ms=round(statistics.median([x for b in blocks for x in b]), 4),
                                 per_round_median_ms=[round(statistics.median(b), 4) for b in blocks])
    out["rate"] = dict(cameras=n_cameras, rows_agreeing_with_torch_to_1e_4=agree, **rate_ms,
                       bytes_per_gaussian=16, copy_bytes_per_gaussian=16,
                       rate_over_copy=round(rate_ms["rate"]["median_ms"] / rate_ms["copy"]["median_ms"], 2),
                       torch_over_rate=round(rate_ms["torch"]["median_ms"] / rate_ms["rate"]["median_ms"], 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["D", "B"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cameras", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "filter3d_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around the per-Gaussian entry points and around fused.rasterize + backward, alternating "
                      "antialiased / antialiased + filter3d blocks of one process after a spin-up; gs_filter3d_rate over "
                      "all cameras against the per-camera PyTorch composition and a copy of its 16 bytes per Gaussian; ms",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.rounds, args.reps, args.cameras)
        r = record["workloads"][w]
        print(json.dumps({w: {k: r[k] for k in ("median_ms", "unfiltered_spread_ms", "filtered_minus_unfiltered_ms",
                                                "rate")}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
