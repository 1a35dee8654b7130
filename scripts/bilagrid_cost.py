"""What the bilateral-grid colour correction costs (csrc/bilagrid.hip, gaussian_splatting_amd/bilagrid.py): each of the
three kernels next to a stream copy of its own algorithmic bytes and next to the PyTorch composition of the same step,
and the loss step with and without the slice in front of it.

    python scripts/bilagrid_cost.py [--sizes 1297x840 1920x1080] [--grid 8 16 16] [--images 200] [--rounds 6] [--reps 10]
                                    [--out profiles/r23/bilagrid_cost.json]

One process, events on the current stream (gaussian_splatting_amd._hip), alternating blocks: every round runs, per size,
one block of `--reps` calls of every item in turn.  Every call of an item works on the next of a ring of buffer sets
whose total exceeds twice the 256 MiB Infinity Cache (at least three sets), so no call finds its image there.

  slice            gs_bilagrid_slice: 12 B read + 12 B written per pixel       copy of 12 HW bytes (24 HW of traffic)
  slice_backward   gs_bilagrid_slice_backward, both gradients: image and       copy of 24 HW bytes (48 HW of traffic)
                   grad_out read by the one kernel, grad_image written (36 B;
                   the yardstick's 48 B count a second read of both)
                   (_image_only / _grid_only: the same call with the other output NULL)
  tv               gs_bilagrid_tv, value and gradient, `--images` grids:       copy of 4 n bytes (8 n of traffic)
                   4 B read + 4 B written per grid element
  pytorch_*        the same step as PyTorch calls: 5-D grid_sample(bilinear, align_corners, border) plus the affine, its
                   autograd backward over a graph built outside the timed region, the index-select total variation
                   forward and backward
  loss_step*       train_ops.ssim_l1_loss(x, target).backward() with x = bil(image, i) and with x = image (image requires
                   a gradient in both), GPU time between events around forward and backward

Per item the record holds the median and minimum over all blocks and the per-block medians, and per size the ratios
kernel / copy (the project's yardstick for a plain walk is 1.5) and PyTorch / kernel (recorded, not asserted)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BLOCKS = 4096
RING_BYTES = 2 * 256 * 2 ** 20 + 2 ** 27


def slice_torch(grid, image):
    """grid_sample over (gx, gy, luma) and the affine: the composition a PyTorch trainer runs"""
    import torch
    _, L, Hg, Wg = grid.shape
    H, W, _ = image.shape
    gx = (torch.arange(W, device=image.device, dtype=torch.float32) + 0.5) / W * 2 - 1
    gy = (torch.arange(H, device=image.device, dtype=torch.float32) + 0.5) / H * 2 - 1
    lum = (0.299 * image[..., 0] + 0.587 * image[..., 1]) + 0.114 * image[..., 2]
    coords = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W), lum.clamp(0, 1) * 2 - 1], -1)[None, None]
    A = torch.nn.functional.grid_sample(grid[None], coords, mode="bilinear", align_corners=True, padding_mode="border")
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * image[..., None, :]).sum(-1) + A[..., 3]


def tv_torch(grids):
    import torch
    val = 0
    for ax in (2, 3, 4):
        n = grids.shape[ax]
        if n >= 2:
            hi = grids.index_select(ax, torch.arange(1, n, device=grids.device))
            lo = grids.index_select(ax, torch.arange(0, n - 1, device=grids.device))
            val = val + ((hi - lo) ** 2).mean()
    return val


def measure(W, H, grid_shape, n_images, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip, bilagrid, train_ops
    dev = torch.device("cuda", 0)
    L, Hg, Wg = grid_shape
    gen = torch.Generator(device=dev).manual_seed(W + H)
    P = H * W
    n_sets = max(3, -(-RING_BYTES // (36 * P)))
    eye = torch.eye(3, 4, device=dev).reshape(12, 1, 1, 1)
    grid = (eye + 0.1 * torch.randn(12, L, Hg, Wg, device=dev, generator=gen)).contiguous()
    sets = []
    for _ in range(n_sets):
        image = torch.rand(H, W, 3, device=dev, generator=gen)
        sets.append(dict(image=image, grad_out=torch.randn(H, W, 3, device=dev, generator=gen), out=torch.empty_like(image),
                         grad_image=torch.empty_like(image), target=torch.rand(H, W, 3, device=dev, generator=gen),
                         src2=torch.rand(6 * P, device=dev, generator=gen), dst2=torch.empty(6 * P, device=dev)))
    grad_grid = torch.empty_like(grid)
    ws = torch.empty(max(_hip.lib().gs_bilagrid_workspace_bytes(H, W, L, Hg, Wg) // 4, 1), device=dev)
    n_tv = n_images * 12 * L * Hg * Wg
    tv_sets = max(3, -(-RING_BYTES // (8 * n_tv)))
    stacks = [(eye[None] + 0.1 * torch.randn(n_images, 12, L, Hg, Wg, device=dev, generator=gen)).contiguous()
              for _ in range(tv_sets)]
    tv_grads = [torch.empty_like(s) for s in stacks]
    tv_ws = torch.empty(_hip.lib().gs_bilagrid_tv_workspace_bytes(n_images, L, Hg, Wg) // 8, dtype=torch.float64, device=dev)
    tv_out = torch.empty(1, device=dev)
    bil = bilagrid.BilateralGrid(3, Wg, Hg, L, device=dev)
    with torch.no_grad():
        bil.grids[1] = grid
    # graphs of the PyTorch composition, built once per set outside the timed region
    graphs = []
    for s in sets[:3]:
        g, i = grid.clone().requires_grad_(True), s["image"].clone().requires_grad_(True)
        graphs.append((slice_torch(g, i), s["grad_out"], g, i))
    stream = _hip.current_stream()
    p = _hip.ptr
    turn = {}

    def nxt(name, ring):
        turn[name] = turn.get(name, -1) + 1
        return ring[turn[name] % len(ring)]

    def k_slice():
        s = nxt("slice", sets)
        _hip.call("gs_bilagrid_slice", p(grid), p(s["image"]), H, W, L, Hg, Wg, p(s["out"]), stream)

    def k_bwd():
        s = nxt("bwd", sets)
        _hip.call("gs_bilagrid_slice_backward", p(grid), p(s["image"]), p(s["grad_out"]), H, W, L, Hg, Wg, p(ws),
                  p(s["grad_image"]), p(grad_grid), stream)

    def k_bwd_part(name, want_image, want_grid):
        s = nxt(name, sets)
        _hip.call("gs_bilagrid_slice_backward", p(grid), p(s["image"]), p(s["grad_out"]), H, W, L, Hg, Wg, p(ws),
                  p(s["grad_image"]) if want_image else None, p(grad_grid) if want_grid else None, stream, label=name)

    def k_tv():
        i = turn["tv"] = turn.get("tv", -1) + 1
        _hip.call("gs_bilagrid_tv", p(stacks[i % tv_sets]), n_images, L, Hg, Wg, p(tv_ws), p(tv_out),
                  p(tv_grads[i % tv_sets]), stream)

    def copy(name, nbytes, src, dst):
        s = nxt(name, sets)
        _hip.call("gs_stream_copy", p(s[dst]), p(s[src]), nbytes - nbytes % 16, COPY_BLOCKS, stream, label=name)

    def copy_tv():
        i = turn["ctv"] = turn.get("ctv", -1) + 1
        _hip.call("gs_stream_copy", p(tv_grads[i % tv_sets]), p(stacks[i % tv_sets]), 4 * n_tv - (4 * n_tv) % 16,
                  COPY_BLOCKS, stream, label="copy_tv")

    def copy_bwd():
        s = nxt("cbwd", sets)
        _hip.call("gs_stream_copy", p(s["dst2"]), p(s["src2"]), 24 * P - (24 * P) % 16, COPY_BLOCKS, stream,
                  label="copy_slice_backward")

    def t_slice():
        s = nxt("tslice", sets)
        with torch.no_grad():
            _hip.timed_region("pytorch_slice", lambda: slice_torch(grid, s["image"]))

    def t_bwd():
        out, go, g, i = nxt("tbwd", graphs)
        g.grad = i.grad = None   # assigned, not accumulated into
        _hip.timed_region("pytorch_slice_backward", lambda: out.backward(go, retain_graph=True))

    def t_tv():
        g = nxt("ttv", stacks).detach().requires_grad_(True)
        _hip.timed_region("pytorch_tv", lambda: tv_torch(g).backward())

    def loss_step(name, with_bil):
        s = nxt(name, sets)
        img = s["image"].detach().requires_grad_(True)

        def step():
            x = bil(img, 1) if with_bil else img
            train_ops.ssim_l1_loss(x, s["target"]).backward()
        _hip.timed_region(name, step)
        bil.grids.grad = None

    items = {
        "slice": ("gs_bilagrid_slice", k_slice),
        "copy_slice": ("copy_slice", lambda: copy("copy_slice", 12 * P, "image", "out")),
        "slice_backward": ("gs_bilagrid_slice_backward", k_bwd),
        "copy_slice_backward": ("copy_slice_backward", copy_bwd),
        "slice_backward_image_only": ("slice_backward_image_only",
                                      lambda: k_bwd_part("slice_backward_image_only", True, False)),
        "slice_backward_grid_only": ("slice_backward_grid_only", lambda: k_bwd_part("slice_backward_grid_only", False, True)),
        "tv": ("gs_bilagrid_tv", k_tv),
        "copy_tv": ("copy_tv", copy_tv),
        "pytorch_slice": ("pytorch_slice", t_slice),
        "pytorch_slice_backward": ("pytorch_slice_backward", t_bwd),
        "pytorch_tv": ("pytorch_tv", t_tv),
        "loss_step_with_bilagrid": ("loss_step_with_bilagrid", lambda: loss_step("loss_step_with_bilagrid", True)),
        "loss_step": ("loss_step", lambda: loss_step("loss_step", False)),
    }

    def block(fn, name, count):
        _hip.enable_timing(True, only=name)   # the calls inside a timed region are not bracketed themselves
        for _ in range(count):
            fn()
        ms = _hip.collect_timing()[name]
        _hip.enable_timing(False)
        return ms

    for _, fn in items.values():   # warm-up: every item twice
        fn(), fn()
    torch.cuda.synchronize()
    _hip.reserve_events(2 * reps)
    blocks = {k: [] for k in items}
    for _ in range(rounds):
        for k, (name, fn) in items.items():
            blocks[k].append(block(fn, name, reps))

    def summary(bs):
        pooled = [x for blk in bs for x in blk]
        return dict(median_ms=round(statistics.median(pooled), 4), min_ms=round(min(pooled), 4),
                    block_median_ms=[round(statistics.median(blk), 4) for blk in bs])

    out = {k: summary(v) for k, v in blocks.items()}
    traffic = {"slice": 24 * P, "copy_slice": 24 * P, "slice_backward": 36 * P, "copy_slice_backward": 48 * P,
               "tv": 8 * n_tv, "copy_tv": 8 * n_tv}
    for k, nbytes in traffic.items():
        out[k]["traffic_bytes"] = nbytes
        out[k]["gbs"] = round(nbytes / out[k]["median_ms"] / 1e6, 1)
    med = lambda k: out[k]["median_ms"]
    out["buffer_sets"], out["tv_buffer_sets"] = n_sets, tv_sets
    out["workspace_bytes"] = int(ws.numel() * 4)
    for k in ("slice", "slice_backward", "tv"):
        out[f"{k}_over_copy"] = round(med(k) / med(f"copy_{k}"), 3)
        out[f"pytorch_over_{k}"] = round(med(f"pytorch_{k}") / med(k), 2)
    out["loss_step_added_ms"] = round(med("loss_step_with_bilagrid") - med("loss_step"), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1297x840", "1920x1080"])
    ap.add_argument("--grid", type=int, nargs=3, default=[8, 16, 16], metavar=("L", "HG", "WG"))
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "bilagrid_cost.json"))
    args = ap.parse_args()
    record = {"what": "events on the current stream, one process, alternating blocks per round and size; every call of an "
                      "item takes the next of a ring of buffer sets larger than twice the Infinity Cache.  slice / "
                      "slice_backward (both gradients) / tv (value and gradient) against gs_stream_copy of 12 HW / 24 HW / "
                      "4 n bytes and against the PyTorch composition (grid_sample and the affine, its autograd backward over "
                      "a prebuilt graph, the index-select total variation forward and backward); "
                      "ssim_l1_loss(x).backward() with x = bil(image, 1) and x = image",
              "grid_L_Hg_Wg": args.grid, "tv_images": args.images, "rounds": args.rounds, "reps": args.reps, "sizes": {}}
    for size in args.sizes:
        W, H = (int(v) for v in size.split("x"))
        r = record["sizes"][size] = measure(W, H, tuple(args.grid), args.images, args.rounds, args.reps)
        print(json.dumps({size: {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in r.items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(os.path.abspath(args.out), ROOT)}))


if __name__ == "__main__":
    main()
