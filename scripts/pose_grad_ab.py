"""What camera_T_world's gradient costs, and that the plain frame does not move.

  python scripts/pose_grad_ab.py --out profiles/r08/pose_grad_D.json [--workload D] [--parent DIR] [--variant-lib SO]

Every measurement runs in a child process of its own (a time limit each; the first failure ends the run):
  ab      one process, after warm-up: BLOCKS alternating blocks of ITERS frames (forward + backward, device events)
          with the pose a constant ("plain") and with the pose requiring grad ("pose"); then the GPU time of
          gs_pose_backward alone (events around the entry point: k_pose_bwd + k_pose_sum) and the bytes it moves
  plain   the plain frame alone, --rounds times, alternating with the same measurement of the tree at --parent (a
          built checkout of the parent commit) when given: the plain frame launches nothing new, so it must stay inside
          the parent's own run-to-run spread
  stage   gs_pose_backward alone on the frame's buffers and a random slab, ITERS calls (events around each), --rounds
          times, alternating with --variant-lib when given: another build of the library (GSPLAT_HIP_LIB), e.g. one
          whose POSE_MAX_BLOCKS is out of reach, i.e. one Gaussian per thread
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS, ITERS, WARMUP = 5, 40, 30


def child(mode, root, workload):
    sys.path.insert(0, root)
    import torch

    from gaussian_splatting_amd import _hip, fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene

    N, W, H, deg = WORKLOADS[workload]
    dev = "cuda"
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    names = [k for k in ("xyz", "quaternion", "scale", "opacity", "rgb", "sh") if getattr(g, k) is not None]
    for k in names:
        getattr(g, k).requires_grad_(True)
    bg = torch.full((3,), 0.5, device=dev)
    gi = make_grad_image(W, H, seed=1, device=dev)
    T_pose = T.clone().requires_grad_(True)

    def frame(pose):
        for k in names:
            getattr(g, k).grad = None
        T_pose.grad = None
        img, mask, uv = fused.rasterize(g, T_pose if pose else T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
        img.backward(gi)
        return mask

    def block(pose, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            frame(pose)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    out = dict(mode=mode, workload=workload, N=N, iters_per_block=ITERS)
    if mode == "stage":
        with torch.no_grad():
            f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H,
                                         DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                                         DEFAULTS["mh_dist"], None, 0)
            slab = torch.randn(max(f.V, 1), 9, device=dev) * 1e-3
            for _ in range(WARMUP):
                fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)
            _hip.enable_timing(True, only="gs_pose_backward")
            for _ in range(ITERS):
                fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)
            ms = _hip.collect_timing()["gs_pose_backward"]
            _hip.enable_timing(False)
        out.update(V=f.V, workgroup_rows=(_hip.lib().gs_pose_workspace_floats(N) - 4) // 12, lib=_hip.LIB_PATH,
                   ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))
        print("RESULT " + json.dumps(out), flush=True)
        return
    for _ in range(WARMUP):
        frame(False)
    if mode == "plain":
        out["plain_ms"] = [block(False, ITERS) for _ in range(BLOCKS)]
    else:
        for _ in range(WARMUP):
            frame(True)
        plain, pose = [], []
        for _ in range(BLOCKS):
            plain.append(block(False, ITERS))
            pose.append(block(True, ITERS))
        out["plain_ms"], out["pose_ms"] = plain, pose
        _hip.reserve_events(4 * ITERS)
        _hip.enable_timing(True, only="gs_pose_backward")
        for _ in range(ITERS):
            mask = frame(True)
        ms = _hip.collect_timing()["gs_pose_backward"]
        _hip.enable_timing(False)
        V = int((~mask).sum())
        # xyz 12 + quaternion 16 + scale 12 + rank 4 per Gaussian of the visible ones' cache lines, slab 36 per visible
        # one; every Gaussian's rank is read
        nbytes = 76 * V + 4 * N
        med = statistics.median(ms)
        out.update(V=V, pose_backward_ms_median=med, pose_backward_ms_min=min(ms), pose_backward_ms_max=max(ms),
                   pose_backward_bytes=nbytes, pose_backward_GBps=nbytes / (med * 1e-3) / 1e9,
                   orchestration=fused.counters()["orchestration"])
    print("RESULT " + json.dumps(out), flush=True)


def run_child(mode, root, workload, lib=None):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root,
           "--workload", workload]
    env = dict(os.environ)
    if lib:
        env["GSPLAT_HIP_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{mode} in {root} ended with status {p.returncode}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    print(f"done: {mode} in {root}" + (f" with {lib}" if lib else ""), file=sys.stderr, flush=True)
    return json.loads(line[len("RESULT "):])


def spread(blocks):
    return dict(median=statistics.median(blocks), min=min(blocks), max=max(blocks), blocks=blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--workload", default="D")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--variant-lib", default=None, help="another build of libgsplat_hip.so to time gs_pose_backward with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=os.path.dirname(HERE))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.workload)
    this_runs, parent_runs = [], []
    for _ in range(a.rounds):
        if a.parent:
            parent_runs.append(run_child("plain", os.path.abspath(a.parent), a.workload)["plain_ms"])
        this_runs.append(run_child("plain", a.root, a.workload)["plain_ms"])
    ab = run_child("ab", a.root, a.workload)
    flat = lambda runs: [x for r in runs for x in r]
    res = dict(what="frame = fused.rasterize forward + backward, ms per frame over blocks of %d frames (device events); "
                    "plain: camera_T_world a constant, pose: it requires grad" % ITERS,
               workload=a.workload, ab=dict(plain_ms=spread(ab.pop("plain_ms")), pose_ms=spread(ab.pop("pose_ms")), **ab),
               plain_this_tree=dict(per_process_median=[statistics.median(r) for r in this_runs], **spread(flat(this_runs))))
    if parent_runs:
        res["plain_parent_commit"] = dict(per_process_median=[statistics.median(r) for r in parent_runs],
                                          **spread(flat(parent_runs)))
    stage = {"this_build": [], "variant_lib": []}
    for _ in range(a.rounds):
        stage["this_build"].append(run_child("stage", a.root, a.workload))
        if a.variant_lib:
            stage["variant_lib"].append(run_child("stage", a.root, a.workload, lib=a.variant_lib))
    res["stage_gs_pose_backward"] = {k: dict(workgroup_rows=v[0]["workgroup_rows"], V=v[0]["V"],
                                             ms_median_per_process=[x["ms_median"] for x in v],
                                             ms_min=min(x["ms_min"] for x in v), ms_max=max(x["ms_max"] for x in v))
                                     for k, v in stage.items() if v}
    res["ab"]["pose_minus_plain_ms"] = res["ab"]["pose_ms"]["median"] - res["ab"]["plain_ms"]["median"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
