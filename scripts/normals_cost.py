"""What the normals cost: the four kernels of csrc/normals.hip against a stream copy of their bytes and
against their PyTorch compositions, and fused.rasterize_normals against fused.rasterize_features with four channels, at
workloads D and B.

    python scripts/normals_cost.py [--workloads D B] [--rounds 6] [--reps 10] [--out profiles/r20/normals_cost.json]

One process: per workload the scene once, a spin-up, then `--rounds` alternating blocks of `--reps` iterations, events
around each call:
  gaussian_normals / _backward   the entry points on the frame's visible rows; copy: gs_stream_copy of the same byte
                                 count (forward 56 B per visible row: vis_idx 4, quaternion 16, scale 12, xyz_cam 12 in,
                                 12 out; backward 4 + 16 per Gaussian plus 16 + 12 + 12 + 12 per visible one: rank and
                                 grad_quaternion for all, quaternion, scale, xyz_cam and grad_normals for the visible)
  depth_normal / _backward       the entry points on the frame's own depth and alpha; copy: 20 B per pixel (forward 8 in,
                                 12 out; backward 8 + 12 in, 8 out = 28 B per pixel)
  torch                          the PyTorch composition of each op (its autograd backward for the two backwards)
  frame                          rasterize_normals + backward of a loss on all four maps against rasterize_features
                                 (C = 4) + the same loss on image, feature_map, alpha
A copy of B bytes moves B / 2 in and B / 2 out, so its time is what a kernel that reads and writes B bytes in all is
held against; plain walks are allowed 1.5 times it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_blocks(fns, rounds, reps):
    """alternating blocks: per round, each fn of the dict `reps` times -> {name: [per-round lists of ms]}"""
    import torch
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            pairs = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                pairs.append((a, b))
            torch.cuda.synchronize()
            out[name].append([a.elapsed_time(b) for a, b in pairs])
    return out


def summary(blocks):
    return {k: dict(median_ms=round(statistics.median([x for b in v for x in b]), 4),
                    min_ms=round(min(x for b in v for x in b), 4),
                    per_round_median_ms=[round(statistics.median(b), 4) for b in v]) for k, v in blocks.items()}


def torch_gaussian_normals(q, s, T, vis, p):
    import torch
    q, s = q[vis], s[vis]
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    axis = s.argmin(dim=1)
    n = torch.gather(R, 2, axis[:, None, None].expand(-1, 3, 1)).squeeze(2) @ T[:3, :3].t()
    return torch.where(((n * p).sum(dim=1) > 0)[:, None], -n, n)


def torch_depth_normal(depth, alpha, K):
    import torch
    H, W = depth.shape
    has = alpha > 0
    d = depth / torch.where(has, alpha, torch.ones_like(alpha))
    x = torch.arange(W, device=depth.device, dtype=torch.float32)[None, :]
    y = torch.arange(H, device=depth.device, dtype=torch.float32)[:, None]
    P = torch.stack([d * (x - K[0, 2]) / K[0, 0], d * (y - K[1, 2]) / K[1, 1], d], dim=2)
    c = torch.linalg.cross(P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2], dim=2)
    n2 = (c * c).sum(dim=2)
    ok = has[1:-1, 1:-1] & has[2:, 1:-1] & has[:-2, 1:-1] & has[1:-1, 2:] & has[1:-1, :-2] & (n2 > 0)
    n = torch.where(ok[:, :, None], c / torch.sqrt(torch.where(ok, n2, torch.ones_like(n2)))[:, :, None], torch.zeros_like(c))
    return torch.nn.functional.pad(n, (0, 0, 1, 1, 1, 1))


def measure(workload, rounds, reps):
    import ctypes

    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_scene
    dev = torch.device("cuda", 0)
    N, W, H, deg = WORKLOADS[workload]
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    bg = torch.zeros(3, device=dev)
    d = DEFAULTS
    names = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, 0)
    V = f.V
    vis = f.vis_idx[:V].contiguous()
    vis_long = vis.long()
    xyz_cam = f.xyz_cam[:V].contiguous()
    with torch.no_grad():
        _, depth, alpha, _, _, _ = fused.rasterize_normals(g, T, cam, use_sh_precompute=True, background_rgb=bg, **d)
    depth, alpha = depth.contiguous(), alpha.contiguous()
    gen = torch.Generator().manual_seed(3)
    g_n = torch.randn(V, 3, generator=gen).to(dev)
    g_map = torch.randn(H, W, 3, generator=gen).to(dev)
    mode = _hip.GS_RASTER_CLASSIC
    stream = _hip.current_stream()
    bytes_of = {"gaussian_normals": 56 * V, "gaussian_normals_backward": 20 * N + 52 * V,
                "depth_normal": 20 * H * W, "depth_normal_backward": 28 * H * W}
    biggest = max(bytes_of.values()) // 2 + 64
    src, dst = torch.empty(biggest, dtype=torch.uint8, device=dev), torch.empty(biggest, dtype=torch.uint8, device=dev)

    def copy_of(n_bytes):
        half = (n_bytes // 2 + 15) // 16 * 16   # the copy reads half and writes half
        return lambda: _hip.call("gs_stream_copy", ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                 ctypes.c_size_t(half), 4096, stream)

    q_leaf = g.quaternion.detach().clone().requires_grad_(True)
    d_leaf, a_leaf = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)

    def torch_bwd_normals():
        q_leaf.grad = None
        (torch_gaussian_normals(q_leaf, g.scale, T, vis_long, xyz_cam) * g_n).sum().backward()

    def torch_bwd_depth():
        d_leaf.grad, a_leaf.grad = None, None
        (torch_depth_normal(d_leaf, a_leaf, cam.K) * g_map).sum().backward()

    kernels = {
        "gaussian_normals": dict(
            kernel=lambda: fused.gaussian_normals_forward(g.quaternion, g.scale, T, vis, xyz_cam),
            torch=lambda: torch_gaussian_normals(g.quaternion, g.scale, T, vis_long, xyz_cam)),
        "gaussian_normals_backward": dict(
            kernel=lambda: fused.gaussian_normals_backward(g.quaternion, g.scale, T, f.rank, xyz_cam, g_n),
            torch=torch_bwd_normals),   # (forward + backward: autograd has no backward alone)
        "depth_normal": dict(
            kernel=lambda: fused.depth_normal_forward(depth, alpha, cam.K, 0.0, mode),
            torch=lambda: torch_depth_normal(depth, alpha, cam.K)),
        "depth_normal_backward": dict(
            kernel=lambda: fused.depth_normal_backward(depth, alpha, cam.K, g_map, 0.0, mode),
            torch=torch_bwd_depth)}
    out = dict(workload=workload, N=N, W=W, H=H, sh_degree=deg, V=V, kernels={})
    with torch.no_grad():
        agree = float(((fused.gaussian_normals_forward(g.quaternion, g.scale, T, vis, xyz_cam) -
                        torch_gaussian_normals(g.quaternion, g.scale, T, vis_long, xyz_cam)).abs().max(dim=1).values < 1e-4)
                      .float().mean())
    out["normals_rows_agreeing_with_torch_to_1e_4"] = agree
    for name, fns in kernels.items():
        fns = dict(fns, copy=copy_of(bytes_of[name]))
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        res = summary(timed_blocks(fns, rounds, reps))
        res["bytes"] = bytes_of[name]
        res["kernel_over_copy"] = round(res["kernel"]["median_ms"] / res["copy"]["median_ms"], 2)
        res["torch_over_kernel"] = round(res["torch"]["median_ms"] / res["kernel"]["median_ms"], 1)
        res["kernel_gbs"] = round(bytes_of[name] / (res["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        out["kernels"][name] = res
    # ---- the frame: rasterize_normals against rasterize_features with C = 4 ----
    for k in names:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    feat = torch.randn(N, 4, generator=gen).to(dev).requires_grad_(True)
    w = torch.randn(H, W, 8, generator=gen).to(dev) / (W * H)

    def clear():
        for k in names:
            if getattr(g, k) is not None:
                getattr(g, k).grad = None
        feat.grad = None

    def normals_frame():
        clear()
        image, dep, al, nm, _, _ = fused.rasterize_normals(g, T, cam, use_sh_precompute=True, background_rgb=bg, **d)
        ((image * w[..., :3]).sum() + (nm * w[..., 3:6]).sum() + (dep * w[..., 6]).sum() + (al * w[..., 7]).sum()).backward()

    def features_frame():
        clear()
        image, fm, al, _, _ = fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=bg, **d)
        ((image * w[..., :3]).sum() + (fm * w[..., 3:7]).sum() + (al * w[..., 7]).sum()).backward()

    fns = {"rasterize_features_C4": features_frame, "rasterize_normals": normals_frame}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = summary(timed_blocks(fns, rounds, reps))
    res["normals_minus_features_ms"] = round(res["rasterize_normals"]["median_ms"] - res["rasterize_features_C4"]["median_ms"], 4)
    spread = res["rasterize_features_C4"]["per_round_median_ms"]
    res["features_spread_ms"] = round(max(spread) - min(spread), 4)
    res["two_normals_launches_ms"] = round(out["kernels"]["gaussian_normals"]["kernel"]["median_ms"] +
                                           out["kernels"]["gaussian_normals_backward"]["kernel"]["median_ms"], 4)
    out["frame"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["D", "B"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "normals_cost.json"))
    args = ap.parse_args()
    record = {"what": "events around each call, alternating blocks of one process after a spin-up: the four kernels of "
                      "csrc/normals.hip, a gs_stream_copy moving the same bytes, their PyTorch compositions, and "
                      "rasterize_normals against rasterize_features with four channels (forward + backward); ms",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for wl in args.workloads:
        r = measure(wl, args.rounds, args.reps)
        record["workloads"][wl] = r
        print(json.dumps({wl: {"kernels": {k: {x: v[x] for x in ("kernel_over_copy", "torch_over_kernel", "kernel_gbs")}
                                           | {"kernel_ms": v["kernel"]["median_ms"]} for k, v in r["kernels"].items()},
                               "frame": {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in r["frame"].items()}}}),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
