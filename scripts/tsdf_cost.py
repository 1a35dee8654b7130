"""What the TSDF fusion and the mesh extraction cost (csrc/tsdf.hip, gaussian_splatting_amd/mesh.py): gs_tsdf_integrate
for one view and for a batch next to a stream copy of the bytes the launch moves and next to the PyTorch composition of
the same update, one extraction of the fused volume, and what the fused surface of a synthetic scene looks like.

    python scripts/tsdf_cost.py [--dims 256 256 256] [--size 1297x840] [--batch 8] [--rounds 5] [--reps 6]
                                [--out profiles/r24/tsdf_cost.json]

One process, events on the current stream (gaussian_splatting_amd._hip), alternating blocks: every round runs one block
of `--reps` calls of every item in turn.  Every call of an item works on the next of a ring of three volumes; one
coloured 256^3 volume is 320 MiB, more than the 256 MiB Infinity Cache, so no call finds its volume there.

  integrate_1 / _C     gs_tsdf_integrate with 1 / C views on a coloured volume: 20 B read per node, 20 B written per node
                       that a view updates (the share is counted once and recorded)
  copy_1 / _C          gs_stream_copy moving the same number of bytes (half read, half written)
  pytorch_1 / _C       the same update as PyTorch calls on the whole volume, view after view
  extract              TSDFVolume.extract_mesh of the volume after the C views: count, two scans, the host read, emit
  surface              Gaussian discs on a unit sphere rendered from 14 views through mesh.integrate_frame into a 128^3
                       volume: the radial error of the mesh's vertices, in voxels (a measured figure, not a gate)

The views stand on a circle around the volume's centre and see a sphere in front of a wall behind the volume, so every
node inside a frustum is updated (carved free or inside the band).  Per item the record holds the median and minimum
over all blocks and the per-block medians; the ratios kernel / copy (the project's yardstick for a plain walk is 1.5)
and PyTorch / kernel are recorded, not asserted."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BLOCKS = 4096


def look_at(eye, target, dev):
    """camera_T_world [4, 4] float32 of a camera at eye looking at target, y down"""
    import torch
    eye, target = (torch.tensor(v, dtype=torch.float64) for v in (eye, target))
    fwd = target - eye
    fwd = fwd / fwd.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.stack([right, down, fwd])
    M[:3, 3] = -M[:3, :3] @ eye
    return M.float().to(dev)


def sphere_depth(M, K, W, H, centre, radius, wall, dev):
    """camera-frame z of a sphere in front of the plane z_cam = wall, pinhole, integer pixel coordinates"""
    import torch
    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    ray = torch.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], torch.ones_like(px)], -1)
    c = M[:3, :3] @ torch.tensor(centre, dtype=torch.float32, device=dev) + M[:3, 3]
    A, B = (ray * ray).sum(-1), ray @ c
    disc = B * B - A * (c @ c - radius * radius)
    return torch.where(disc > 0, (B - disc.clamp(min=0).sqrt()) / A, torch.full_like(A, wall))


def integrate_torch(vol, depths, images, cams, Ks, near):
    """the update of gs_tsdf_integrate (pinhole) as PyTorch calls over the whole volume, view after view, in place"""
    import torch
    nx, ny, nz = vol.dims
    dev = vol.tsdf.device
    ar = lambda n, o: o + vol.voxel_size * torch.arange(n, device=dev, dtype=torch.float32)
    X, Y, Z = ar(nx, vol.origin[0])[None, None, :], ar(ny, vol.origin[1])[None, :, None], ar(nz, vol.origin[2])[:, None, None]
    C, H, W = depths.shape
    for c in range(C):
        M, K = cams[c], Ks[c]
        c0 = M[0, 0] * X + M[0, 1] * Y + M[0, 2] * Z + M[0, 3]
        c1 = M[1, 0] * X + M[1, 1] * Y + M[1, 2] * Z + M[1, 3]
        c2 = M[2, 0] * X + M[2, 1] * Y + M[2, 2] * Z + M[2, 3]
        fu = torch.floor(K[0, 0] * c0 / c2 + K[0, 2] + 0.5)
        fv = torch.floor(K[1, 1] * c1 / c2 + K[1, 2] + 0.5)
        ok = (c2 > near) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        pix = torch.where(ok, fv * W + fu, torch.zeros_like(fu)).long()
        d = depths[c].reshape(-1)[pix]
        ok &= (d > 0) & torch.isfinite(d)
        sdf = (d - c2) * (torch.sqrt(c0 * c0 + c1 * c1 + c2 * c2) / c2)
        ok &= sdf >= -vol.sdf_trunc
        t = torch.clamp(sdf / vol.sdf_trunc, max=1.0)
        w1 = vol.weight + 1
        vol.tsdf.copy_(torch.where(ok, (vol.tsdf * vol.weight + t) / w1, vol.tsdf))
        rgb = images[c].reshape(-1, 3)[pix]
        vol.color.copy_(torch.where(ok[..., None], (vol.color * vol.weight[..., None] + rgb) / w1[..., None], vol.color))
        vol.weight.copy_(torch.where(ok, torch.clamp(w1, max=vol.max_weight), vol.weight))


def measure(dims, W, H, batch, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip, mesh
    dev = torch.device("cuda", 0)
    nx, ny, nz = dims
    N = nx * ny * nz
    extent = 2.0
    voxel = extent / (max(dims) - 1)
    origin = tuple(-0.5 * voxel * (n - 1) for n in dims)
    vols = [mesh.TSDFVolume(origin, voxel, dims, device=dev) for _ in range(3)]
    K = torch.tensor([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], dtype=torch.float32, device=dev)
    cams, depths, images = [], [], []
    gen = torch.Generator(device=dev).manual_seed(7)
    for c in range(batch):
        a = 2 * math.pi * c / batch
        M = look_at((2.4 * math.sin(a), -0.5, -2.4 * math.cos(a)), (0.0, 0.0, 0.0), dev)
        cams.append(M)
        depths.append(sphere_depth(M, K, W, H, (0.0, 0.0, 0.0), 0.6, 4.5, dev))
        images.append(torch.rand(H, W, 3, device=dev, generator=gen))
    cams, depths, images = torch.stack(cams), torch.stack(depths), torch.stack(images)
    Ks = K[None].repeat(batch, 1, 1).contiguous()
    near = 0.2

    # the share of the nodes a launch writes, counted on a fresh volume
    shares = {}
    for C in (1, batch):
        vols[0].reset()
        vols[0].integrate_views(depths[:C], cams[:C], Ks[:C], images[:C], near_thresh=near)
        shares[C] = float((vols[0].weight > 0).float().mean())
    src = torch.rand(10 * N, device=dev, generator=gen)   # 40 N bytes: the most a launch can move is 20 N read + 20 N written
    dst = torch.empty_like(src)
    traffic = {C: int(20 * N + 20 * N * shares[C]) for C in shares}

    stream = _hip.current_stream()
    p = _hip.ptr
    turn = {}

    def nxt(name):
        turn[name] = turn.get(name, -1) + 1
        return vols[turn[name] % len(vols)]

    def k_integrate(C):
        nxt(f"k{C}").integrate_views(depths[:C], cams[:C], Ks[:C], images[:C], near_thresh=near)

    def copy(C):
        half = traffic[C] // 2
        _hip.call("gs_stream_copy", p(dst), p(src), half - half % 16, COPY_BLOCKS, stream, label=f"copy_{C}")

    def t_integrate(C):
        v = nxt(f"t{C}")
        with torch.no_grad():
            _hip.timed_region(f"pytorch_{C}", lambda: integrate_torch(v, depths[:C], images[:C], cams[:C], Ks[:C], near))

    mesh_counts = {}

    def extract():
        def run():
            v, f, _ = vols[0].extract_mesh()
            mesh_counts["vertices"], mesh_counts["faces"] = int(v.shape[0]), int(f.shape[0])
        _hip.timed_region("extract", run)

    items = {}
    for C in (1, batch):
        items[f"integrate_{C}"] = ("gs_tsdf_integrate", lambda C=C: k_integrate(C))
        items[f"copy_{C}"] = (f"copy_{C}", lambda C=C: copy(C))
        items[f"pytorch_{C}"] = (f"pytorch_{C}", lambda C=C: t_integrate(C))
    items["extract"] = ("extract", extract)

    def block(fn, name, count):
        _hip.enable_timing(True, only=name)
        for _ in range(count):
            fn()
        ms = _hip.collect_timing()[name]
        _hip.enable_timing(False)
        return ms

    for v in vols:   # every volume holds the same fused state when the timing starts
        v.reset()
        v.integrate_views(depths, cams, Ks, images, near_thresh=near)
    for _, fn in items.values():
        fn()
    torch.cuda.synchronize()
    _hip.reserve_events(2 * reps)
    blocks = {k: [] for k in items}
    for _ in range(rounds):
        for k, (name, fn) in items.items():
            blocks[k].append(block(fn, name, reps if not k.startswith("pytorch") and k != "extract" else max(reps // 3, 1)))

    def summary(bs):
        pooled = [x for blk in bs for x in blk]
        return dict(median_ms=round(statistics.median(pooled), 4), min_ms=round(min(pooled), 4),
                    block_median_ms=[round(statistics.median(blk), 4) for blk in bs])

    out = {k: summary(v) for k, v in blocks.items()}
    med = lambda k: out[k]["median_ms"]
    for C in (1, batch):
        for k in (f"integrate_{C}", f"copy_{C}"):
            out[k]["traffic_bytes"] = traffic[C]
            out[k]["gbs"] = round(traffic[C] / med(k) / 1e6, 1)
        out[f"integrate_{C}"]["share_of_nodes_written"] = round(shares[C], 4)
        out[f"integrate_{C}_over_copy"] = round(med(f"integrate_{C}") / med(f"copy_{C}"), 3)
        out[f"pytorch_over_integrate_{C}"] = round(med(f"pytorch_{C}") / med(f"integrate_{C}"), 2)
    out[f"integrate_{batch}_per_view_ms"] = round(med(f"integrate_{batch}") / batch, 4)
    out["extract"].update(mesh_counts)
    out["volume_bytes"] = 20 * N
    return out


def surface(dims=(128, 128, 128), n_gauss=60000, n_views=14, W=640, H=480):
    """Gaussian discs on the unit sphere, fused through mesh.integrate_frame: the radial error of the mesh's vertices"""
    import torch

    from gaussian_splatting_amd import mesh
    from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    n = torch.randn(n_gauss, 3, generator=gen, dtype=torch.float64)
    n = n / n.norm(dim=1, keepdim=True)
    # the rotation taking z to n: q = (1 + n.z, z x n), normalised
    q = torch.stack([1 + n[:, 2], -n[:, 1], n[:, 0], torch.zeros(n_gauss, dtype=torch.float64)], 1)
    q = q / q.norm(dim=1, keepdim=True).clamp(min=1e-12)
    scale = torch.log(torch.tensor([0.02, 0.02, 0.002], dtype=torch.float64)).repeat(n_gauss, 1)
    rgb = (0.5 + 0.5 * n) / 0.28209479177387814
    f32 = lambda t: t.float().to(dev).contiguous()
    g = Gaussians(f32(n), f32(rgb), f32(torch.full((n_gauss, 1), 4.0, dtype=torch.float64)), f32(scale), f32(q), None)
    K = torch.tensor([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], dtype=torch.float32, device=dev)
    cam = Camera(W, H, K)
    voxel = 2.6 / (dims[0] - 1)
    vol = mesh.TSDFVolume((-1.3, -1.3, -1.3), voxel, dims, device=dev)
    bg = torch.zeros(3, device=dev)
    out = {}
    for depth in ("median", "expected"):
        vol.reset()
        for c in range(n_views):
            a, h = 2 * math.pi * c / n_views, (-1.2, 0.0, 1.2)[c % 3]
            M = look_at((3.0 * math.sin(a), h, -3.0 * math.cos(a)), (0.0, 0.0, 0.0), dev)
            mesh.integrate_frame(vol, g, M, cam, 0.2, 100.0, 100, 3.0, bg, depth=depth)
        v, f, _ = vol.extract_mesh(min_weight=2.0)
        err = (v.double().norm(dim=1) - 1.0) / voxel
        # the sphere's outer surface: the discs have a back side too, seen by no camera (weight 0 there)
        out[depth] = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), voxel=round(voxel, 5),
                          radial_error_voxels=dict(mean=round(float(err.mean()), 4), mean_abs=round(float(err.abs().mean()), 4),
                                                   p95_abs=round(float(err.abs().quantile(0.95)), 4),
                                                   max_abs=round(float(err.abs().max()), 4)) if v.shape[0] else None)
    out["scene"] = dict(gaussians=n_gauss, views=n_views, frame=[W, H], dims=list(dims), disc_sigma=[0.02, 0.02, 0.002])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[256, 256, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--size", default="1297x840")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--no-surface", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "tsdf_cost.json"))
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    record = {"what": "events on the current stream, one process, alternating blocks per round; every call of an item takes "
                      "the next of a ring of three coloured volumes, each larger than the Infinity Cache.  gs_tsdf_integrate "
                      "with 1 and C views against gs_stream_copy of the bytes the launch moves (20 B read per node, 20 B "
                      "written per updated node) and against the PyTorch composition of the same update; one extract_mesh "
                      "(count, scans, host read, emit); the fused surface of Gaussian discs on a unit sphere",
              "dims": args.dims, "size": args.size, "batch": args.batch, "rounds": args.rounds, "reps": args.reps}
    record["cost"] = measure(tuple(args.dims), W, H, args.batch, args.rounds, args.reps)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in record["cost"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    write()   # the timings are kept even if the scene below cannot be rendered
    if not args.no_surface:
        record["surface"] = surface()
        print(json.dumps(record["surface"]), flush=True)
        write()
    print(json.dumps({"written": os.path.relpath(os.path.abspath(args.out), ROOT)}))


if __name__ == "__main__":
    main()
