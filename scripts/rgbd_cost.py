"""What the depth / alpha kernels (gs_render_zalpha, gs_render_zalpha_backward) cost next to the colour kernels of the
same frame, at workloads B and D.

    python scripts/rgbd_cost.py [--workloads B D] [--rounds 6] [--reps 10] [--out profiles/r08/rgbd_cost.json] [--no-trace]

One process per run: the per-Gaussian stage, binning and prefix sort once per workload, then `--rounds` alternating
blocks of `--reps` x (colour forward, colour backward) and `--reps` x (depth forward, prologue + depth backward) on
the same lists, events around every C-ABI call (gaussian_splatting_amd._hip.enable_timing); the record holds the median
and the minimum per entry point over all blocks, the per-round medians (the spread) and the depth / colour ratios.
The baseline is the existing colour kernels, not anything rasterize_rgbd adds.  Then, unless --no-trace, one
`rocprofv3 --kernel-trace --stats` pass per workload in a child process of its own, each under its own time limit: the
kernels' own durations (the events above include the launch gaps of an entry point that enqueues several kernels).
A failed or missing trace is recorded as such; the timings stand without it.
"""
import argparse
import json
import os
import sqlite3
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLOUR = ("gs_render_tiles_prefix", "gs_render_tiles_packed", "gs_render_tiles_backward_slab")
DEPTH = ("gs_render_zalpha", "gs_render_zalpha_backward")
KERNELS = ("k_render_zalpha_fwd", "k_render_zalpha_bwd", "k_render_fwd", "k_render_fwd_flagged", "k_render_bwd",
           "k_bwd_prologue")
TRACE_TIMEOUT_S = 420


def frame(workload):
    """the workload's frame up to its sorted lists, and closures for the four passes"""
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

    info = dict(workload=workload, N=N, W=W, H=H, V=V, S=f.S, tiles=f.T, mean_list=round(f.S / max(f.T, 1), 1))
    return colour, depth, state, info


def measure(workload, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip
    colour, depth, state, info = frame(workload)
    for _ in range(3):
        colour()
        depth()
    torch.cuda.synchronize()
    nsp = state["nsp"]
    info["walked_entries"] = int(nsp.sum())        # (pixel, list entry) pairs both walks look at, an upper bound of visits x 64
    info["mean_num_splats"] = round(float(nsp.float().mean()), 1)
    _hip.reserve_events(2 * 8 * reps)
    per_round, pooled = [], {}
    for _ in range(rounds):
        row = {}
        for block in (colour, depth):
            _hip.enable_timing(True)
            for _ in range(reps):
                block()
            for name, ms in _hip.collect_timing().items():
                row[name] = round(statistics.median(ms), 4)
                pooled.setdefault(name, []).extend(ms)
            _hip.enable_timing(False)
        per_round.append(row)
    med = {k: round(statistics.median(v), 4) for k, v in sorted(pooled.items())}
    mn = {k: round(min(v), 4) for k, v in sorted(pooled.items())}
    fwd_colour = sum(med.get(k, 0.0) for k in COLOUR[:2])
    out = dict(info, median_ms=med, min_ms=mn, per_round_median_ms=per_round,
               ratio_forward=round(med["gs_render_zalpha"] / fwd_colour, 3),
               ratio_backward=round(med["gs_render_zalpha_backward"] / med["gs_render_tiles_backward_slab"], 3))
    return out


def child(workload, reps):
    """what one rocprofv3 pass runs: the frame and `reps` x (colour, depth)"""
    import torch
    colour, depth, _, _ = frame(workload)
    for _ in range(reps):
        colour()
        depth()
    torch.cuda.synchronize()


def kernel_stats(db_path):
    db = sqlite3.connect(db_path)
    cur = db.cursor()
    tables = [r[0] for r in cur.execute("select name from sqlite_master where type in ('table', 'view')")]
    table = "kernels" if "kernels" in tables else next(t for t in tables if t.startswith("kernels"))
    cols = [r[1] for r in cur.execute(f"pragma table_info({table})")]
    name_col = "name" if "name" in cols else "kernel_name"
    rows = cur.execute(f"select {name_col}, count(*), avg(end-start), min(end-start) from {table} group by {name_col}").fetchall()
    out = {}
    for name, calls, avg, mn in rows:
        for k in KERNELS:
            if f"gs::{k}<" in name or f"gs::{k}(" in name or name.endswith(f"gs::{k}") or f"{k}E" in name:
                key = name.split("(")[0].replace("void ", "")
                out[key] = dict(calls=calls, mean_us=round(avg / 1e3, 2), min_us=round(mn / 1e3, 2))
    return out


def csv_stats(outdir, name):
    """the same figures from <name>_kernel_stats.csv, for a rocprofv3 that writes CSV instead of a database"""
    import csv
    for base, _, files in os.walk(outdir):
        for fn in files:
            if fn.startswith(name) and fn.endswith("kernel_stats.csv"):
                out = {}
                with open(os.path.join(base, fn), newline="") as fh:
                    for row in csv.DictReader(fh):
                        if any(f"gs::{k}<" in row["Name"] or f"gs::{k}(" in row["Name"] for k in KERNELS):
                            out[row["Name"].split("(")[0].replace("void ", "")] = dict(
                                calls=int(row["Calls"]), mean_us=round(float(row["AverageNs"]) / 1e3, 2),
                                min_us=round(float(row["MinNs"]) / 1e3, 2))
                return out
    return {"error": "no results database or kernel_stats.csv written"}


def trace(workload, outdir, reps):
    """one rocprofv3 pass in a process of its own -> the kernels' durations, or {"error": ...}"""
    os.makedirs(outdir, exist_ok=True)
    name = f"rgbd_{workload}"
    cmd = ["timeout", "-k", "10", str(TRACE_TIMEOUT_S), "rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", name,
           "--", sys.executable, os.path.abspath(__file__), "--child", workload, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-400:]}
    db = None
    for base, _, files in os.walk(outdir):
        for fn in files:
            if fn.startswith(name) and fn.endswith(".db"):
                db = os.path.join(base, fn)
    if db is None:
        return csv_stats(outdir, name)
    try:
        return kernel_stats(db)
    except (sqlite3.Error, StopIteration) as e:
        return {"error": f"{type(e).__name__}: {e}"}
    finally:
        os.remove(db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["B", "D"])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "rgbd_cost.json"))
    ap.add_argument("--trace-dir", default="", help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return
    record = {"what": "events around the C-ABI entry points, alternating blocks of one process; ratio = depth / colour "
                      "(forward: gs_render_zalpha over the colour forward's entry; backward: gs_render_zalpha_backward "
                      "over gs_render_tiles_backward_slab, both without the shared prologue)",
              "rounds": args.rounds, "reps": args.reps, "workloads": {}}
    for w in args.workloads:
        record["workloads"][w] = measure(w, args.rounds, args.reps)
        print(json.dumps({w: {k: record["workloads"][w][k] for k in ("median_ms", "ratio_forward", "ratio_backward")}}),
              flush=True)
    if not args.no_trace:
        import torch
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        import tempfile
        trace_dir = args.trace_dir or tempfile.mkdtemp(prefix="rgbd_trace_")
        for w in args.workloads:
            res = trace(w, trace_dir, 5)
            record["workloads"][w]["kernel_trace_us"] = res
            print(json.dumps({w: res}), flush=True)
            if "error" in res:
                break   # nothing more is started on the GPU after a pass that did not end well
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
