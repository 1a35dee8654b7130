"""A/B of one training iteration with and without the fused optimizer step, in one process:

    A   fused.rasterize -> ssim_l1_loss -> backward -> train_ops.Adam.step -> accumulate_grad_stats
    B   the same with train_ops.FusedRasterAdam (quaternion, scale, opacity, rgb, sh stepped inside the backward)

Alternating blocks after warm-up, device-event time per iteration.  B is accepted as faster when its gain exceeds
the spread of A's own blocks.  The kernel times come from two separate kernel traces (no counters), one per variant:

    python scripts/fused_adam_ab.py --out profiles/r07/fused_adam_D.json          # the A/B run
    rocprofv3 --kernel-trace --stats -d DIR -o a -- python scripts/fused_adam_ab.py --variant A --iters 60
    rocprofv3 --kernel-trace --stats -d DIR -o b -- python scripts/fused_adam_ab.py --variant B --iters 60
    python scripts/rocpd_stats.py DIR/a_results.db DIR/a.csv ; ... b.csv
    python scripts/fused_adam_ab.py --merge-trace DIR/a.csv DIR/b.csv --out profiles/r07/fused_adam_D.json

(scripts/fused_adam_ab.sh runs the five steps.)"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
LRS = (2e-4, 4e-3, 1e-2, 2e-2, 4e-3, 2e-4)   # config.py of the reference: base_lr 0.002 times the group multipliers


def byte_model(N, n_coeff):
    """algorithmic bytes per iteration of the per-Gaussian backward's outputs + the optimizer, from shapes:
    A: the dense gradients written (4 B x 59 at degree 3) + k_adam's 28 B per parameter element;
    B: grad_xyz written + 24 B (p, m, v read and written) per element of the five tensors in the backward kernel
       + k_adam's 28 B per element of xyz"""
    per = 3 + 4 + 3 + 1 + 3 + 3 * (n_coeff - 1)   # parameter elements per Gaussian (59)
    five = per - 3
    a = {"grad_write": 4 * per, "adam": 28 * per}
    b = {"grad_xyz_write": 12, "adam_in_backward": 24 * five, "adam_xyz": 28 * 3}
    return {"A_bytes_per_gaussian": a, "B_bytes_per_gaussian": b, "A_bytes": N * sum(a.values()),
            "B_bytes": N * sum(b.values())}


def build(variant, workload, dev):
    import torch

    import bench
    from gaussian_splatting_amd import fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_scene
    from gaussian_splatting_amd.train_ops import Adam, FusedRasterAdam, accumulate_grad_stats, ssim_l1_loss
    N, W, H, deg = WORKLOADS[workload]
    g, cam, _ = make_scene(N, W, H, deg, seed=0, device=dev)
    names = [k for k in NAMES if getattr(g, k) is not None]
    for k in names:
        getattr(g, k).requires_grad_(True)
    cls = FusedRasterAdam if variant == "B" else Adam
    opt = cls([{"params": getattr(g, k), "lr": lr} for k, lr in zip(NAMES, LRS) if getattr(g, k) is not None])
    poses = bench.camera_poses(24, 4321, dev, moving=True)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    bg = torch.zeros(3, device=dev)
    uv_acc, xyz_acc = torch.zeros(N, 2, device=dev), torch.zeros(N, 3, device=dev)
    count = torch.zeros(N, dtype=torch.int32, device=dev)
    rasterize = opt.rasterize if variant == "B" else fused.rasterize

    def iteration(i):
        opt.zero_grad(set_to_none=True)
        img, culled, uv = rasterize(g, poses[i % 24], cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
        uv.retain_grad()
        ssim_l1_loss(img, target, 0.2).backward()
        opt.step()
        accumulate_grad_stats(uv.grad, culled, g.xyz.grad, cam, uv_acc, xyz_acc, count)

    def check():
        if variant == "B":
            assert opt.last_fallback_reason is None, opt.last_fallback_reason
            assert all(getattr(g, k).grad is None for k in names[1:]) and g.xyz.grad is not None
        assert all(bool(torch.isfinite(getattr(g, k)).all()) for k in names)

    return iteration, check, (N, (deg + 1) ** 2)


def timed_block(iteration, start, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(start, start + iters):
        iteration(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run_ab(args):
    import torch
    dev = torch.device("cuda", 0)
    it_a, check_a, (N, n_coeff) = build("A", args.workload, dev)
    it_b, check_b, _ = build("B", args.workload, dev)
    for i in range(args.warmup):
        it_a(i)
        it_b(i)
    check_a()
    check_b()
    blocks = {"A": [], "B": []}
    pos = args.warmup
    for _ in range(args.blocks):
        blocks["A"].append(timed_block(it_a, pos, args.iters))
        blocks["B"].append(timed_block(it_b, pos, args.iters))
        pos += args.iters
    check_a()
    check_b()
    mean = {k: statistics.fmean(v) for k, v in blocks.items()}
    spread_a = max(blocks["A"]) - min(blocks["A"])
    gain = mean["A"] - mean["B"]
    model = byte_model(N, n_coeff)
    out = {
        "what": "training iteration at workload %s: A = fused.rasterize + Adam.step, B = FusedRasterAdam" % args.workload,
        "device": torch.cuda.get_device_name(0), "workload": args.workload, "gaussians": N,
        "blocks": args.blocks, "iterations_per_block": args.iters, "iterations_each": args.blocks * args.iters,
        "A_block_ms_per_iteration": [round(x, 4) for x in blocks["A"]],
        "B_block_ms_per_iteration": [round(x, 4) for x in blocks["B"]],
        "A_ms_per_iteration": round(mean["A"], 4), "B_ms_per_iteration": round(mean["B"], 4),
        "A_block_spread_ms": round(spread_a, 4), "B_block_spread_ms": round(max(blocks["B"]) - min(blocks["B"]), 4),
        "gain_ms": round(gain, 4), "B_faster_by_more_than_A_spread": bool(gain > spread_a),
        "byte_model": model,
        "byte_model_projected_gain_ms_at_5500_GBs": round((model["A_bytes"] - model["B_bytes"]) / 5.5e12 * 1e3, 4),
    }
    return out


def kernel_rows(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return rows


def merge_trace(args, out):
    a, b = kernel_rows(args.merge_trace[0]), kernel_rows(args.merge_trace[1])

    def pick(rows, key):
        hits = {n: v for n, v in rows.items() if key in n}
        calls = sum(c for c, _ in hits.values())
        return (sum(t for _, t in hits.values()) / calls / 1e6) if calls else None, calls

    model = out.get("byte_model") or byte_model(*args.shape)
    a_bwd, a_calls = pick(a, "k_preprocess_bwd")
    a_adam, _ = pick(a, "k_adam")
    b_bwd, b_calls = pick(b, "k_preprocess_bwd")
    b_adam, _ = pick(b, "k_adam")
    tr = {"source": "rocprofv3 --kernel-trace --stats, one run per variant, mean over all calls (warm-up included)",
          "A": {"k_preprocess_bwd_ms": round(a_bwd, 4), "k_adam_ms": round(a_adam, 4), "calls": a_calls,
                "sum_ms": round(a_bwd + a_adam, 4)},
          "B": {"k_preprocess_bwd_adam_ms": round(b_bwd, 4), "k_adam_xyz_ms": round(b_adam, 4), "calls": b_calls,
                "sum_ms": round(b_bwd + b_adam, 4)}}
    tr["A"]["algorithmic_GBs"] = round(model["A_bytes"] / (tr["A"]["sum_ms"] * 1e-3) / 1e9, 1)
    tr["B"]["algorithmic_GBs"] = round(model["B_bytes"] / (tr["B"]["sum_ms"] * 1e-3) / 1e9, 1)
    tr["gain_ms"] = round(tr["A"]["sum_ms"] - tr["B"]["sum_ms"], 4)
    out["kernel_trace"] = tr
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="D", choices=["A", "B", "C", "D"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="iterations per block (blocks x iters >= 200 each by default)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--variant", choices=["A", "B"], help="run only this variant for --iters iterations (for a trace)")
    ap.add_argument("--merge-trace", nargs=2, metavar=("A.csv", "B.csv"), help="add the kernel-trace section to --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.variant:
        import torch
        iteration, check, _ = build(args.variant, args.workload, torch.device("cuda", 0))
        for i in range(args.iters):
            iteration(i)
        torch.cuda.synchronize()
        check()
        print(f"variant {args.variant}: {args.iters} iterations")
        return
    if args.merge_trace:
        from gaussian_splatting_amd.synthetic import WORKLOADS
        N, _, _, deg = WORKLOADS[args.workload]
        args.shape = (N, (deg + 1) ** 2)
        out = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        out = merge_trace(args, out)
    else:
        out = run_ab(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
