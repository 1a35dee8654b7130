"""What MCMC densification costs (csrc/mcmc.hip, densify.MCMCController): the position noise of every iteration next to
a stream copy of its bytes and next to the PyTorch composition of the same step, and one relocation.

    python scripts/mcmc_cost.py [--n 2860000 100000] [--rounds 6] [--reps 10] [--out profiles/r15/mcmc_cost.json]

One process, events on the current stream (gaussian_splatting_amd._hip), alternating blocks: every round runs, per size,
a block of `--reps` gs_mcmc_add_noise, a block of gs_stream_copy with the same traffic (34 N bytes copied = 68 N bytes
read + written; the kernel reads 56 N and writes 12 N), a block of gs_stream_copy of 68 N bytes (twice the traffic), the
first two again over three sets of buffers in turn (at 2.86 M no call finds its data in the Infinity Cache), a
block of the PyTorch composition (sigmoid, gate, normalised quaternion -> rotation, R diag(exp(scale)), its square, bmm
with the scaled noise, add_), a block of the same composition without the batched 3x3 products (M (M^T e) as broadcast
multiply and sum) and one MCMCController.relocate() with 1 % of the rows dead on the six tensors (widths 3, 4,
3, 1, 3, 45) with Adam moments -- GPU time between events around the whole call, its host read included.  Per item the
record holds the median and minimum over all blocks, the per-block medians and the ratios the expectation of DESIGN.md 7h
is about: noise kernel over equal-traffic copy (expected <= 1.5), from one set of buffers and from the rotating sets, and
PyTorch composition over noise kernel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP, GATE_K, GATE_X0 = 5e5 * 1.6e-4, 100.0, 0.995
COPY_BLOCKS = 4096


def torch_noise(xyz, q, s, logit, noise):
    """the step as PyTorch calls (the composition MCMC implementations on torch use)"""
    import torch
    o = torch.sigmoid(logit)
    gate = torch.sigmoid(GATE_K * ((1.0 - o) - GATE_X0))
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    M = R * torch.exp(s)[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    xyz.add_(torch.bmm(cov, (noise * (gate * STEP))[:, :, None]).squeeze(-1))


def torch_noise_elementwise(xyz, q, s, logit, noise):
    """the same without the two batched 3x3 products (broadcast multiply and sum): the cheapest composition"""
    import torch
    o = torch.sigmoid(logit)
    gate = torch.sigmoid(GATE_K * ((1.0 - o) - GATE_X0))
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    M = R * torch.exp(s)[:, None, :]
    t = (M * (noise * (gate * STEP))[:, :, None]).sum(dim=1)    # M^T e
    xyz.add_((M * t[:, None, :]).sum(dim=2))                    # M (M^T e)


def measure(n, rounds, reps):
    import torch

    from gaussian_splatting_amd import _hip
    from gaussian_splatting_amd.densify import MCMCConfig, MCMCController
    from gaussian_splatting_amd.synthetic import make_scene
    from gaussian_splatting_amd.train_ops import Adam
    dev = torch.device("cuda", 0)
    g, _, _ = make_scene(n, 1297, 840, 3, seed=0, device=dev)
    names = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
    for k in names:
        getattr(g, k).requires_grad_(True)
    opt = Adam([{"params": getattr(g, k), "lr": 1e-3} for k in names])
    for k in names:
        getattr(g, k).grad = torch.zeros_like(getattr(g, k))
    opt.step()   # creates the moments
    opt.zero_grad(set_to_none=True)
    ctrl = MCMCController(g, opt, MCMCConfig(cap_max=max(n, 1_000_000)))
    noise = torch.randn(n, 3, device=dev)
    xyz, q, s, logit = (getattr(g, k).detach() for k in ("xyz", "quaternion", "scale", "opacity"))
    a = torch.empty(68 * n // 4, dtype=torch.float32, device=dev).fill_(1.0)
    b = torch.empty_like(a)
    dead_rows = torch.randperm(n, device=dev)[:n // 100]
    stream = _hip.current_stream()
    p = _hip.ptr

    def kernel():
        _hip.call("gs_mcmc_add_noise", p(xyz), p(q), p(s), p(logit), p(noise), n, STEP, GATE_K, GATE_X0, stream)

    def copy(nbytes):
        _hip.call("gs_stream_copy", p(b), p(a), nbytes, COPY_BLOCKS, stream)

    # the same two over three sets of buffers in turn: 3 x 160 MB of tensors and 3 x 194 MB of copy buffers at 2.86 M, so
    # that no call finds its data in the 256 MiB Infinity Cache
    sets = [(xyz, q, s, logit, noise)] + [tuple(t.clone() for t in (xyz, q, s, logit, noise)) for _ in range(2)]
    pairs = [(a, b)] + [(torch.empty_like(a).fill_(1.0), torch.empty_like(b)) for _ in range(2)]
    turn = [0, 0]

    def kernel_rotating():
        x_, q_, s_, l_, e_ = sets[turn[0] % 3]
        turn[0] += 1
        _hip.call("gs_mcmc_add_noise", p(x_), p(q_), p(s_), p(l_), p(e_), n, STEP, GATE_K, GATE_X0, stream)

    def copy_rotating():
        a_, b_ = pairs[turn[1] % 3]
        turn[1] += 1
        _hip.call("gs_stream_copy", p(b_), p(a_), 34 * n, COPY_BLOCKS, stream)

    def block(fn, name, count):
        _hip.enable_timing(True)
        for _ in range(count):
            fn()
        ms = _hip.collect_timing()[name]
        _hip.enable_timing(False)
        return ms

    def relocate_once():
        logit[dead_rows] = -7.0
        torch.cuda.synchronize()
        return block(lambda: _hip.timed_region("relocate", ctrl.relocate), "relocate", 1)

    kernel(), copy(34 * n), copy(68 * n), torch_noise(xyz, q, s, logit, noise), relocate_once()
    torch_noise_elementwise(xyz, q, s, logit, noise)
    for _ in range(3):
        kernel_rotating(), copy_rotating()
    torch.cuda.synchronize()
    _hip.reserve_events(2 * reps)
    blocks = {k: [] for k in ("gs_mcmc_add_noise", "stream_copy_equal_traffic", "stream_copy_68n_bytes",
                              "gs_mcmc_add_noise_rotating", "stream_copy_equal_traffic_rotating", "pytorch_noise",
                              "pytorch_noise_elementwise", "relocate_1pc_dead")}
    for _ in range(rounds):
        blocks["gs_mcmc_add_noise"].append(block(kernel, "gs_mcmc_add_noise", reps))
        blocks["stream_copy_equal_traffic"].append(block(lambda: copy(34 * n), "gs_stream_copy", reps))
        blocks["stream_copy_68n_bytes"].append(block(lambda: copy(68 * n), "gs_stream_copy", reps))
        blocks["gs_mcmc_add_noise_rotating"].append(block(kernel_rotating, "gs_mcmc_add_noise", reps))
        blocks["stream_copy_equal_traffic_rotating"].append(block(copy_rotating, "gs_stream_copy", reps))
        blocks["pytorch_noise"].append(block(lambda: _hip.timed_region("pytorch_noise", lambda: torch_noise(
            xyz, q, s, logit, noise)), "pytorch_noise", reps))
        blocks["pytorch_noise_elementwise"].append(block(lambda: _hip.timed_region(
            "pytorch_noise_elementwise", lambda: torch_noise_elementwise(xyz, q, s, logit, noise)),
            "pytorch_noise_elementwise", reps))
        blocks["relocate_1pc_dead"].append(relocate_once())
        for x_, *_ in sets:
            x_.clamp_(-1e3, 1e3)   # (the noise accumulates over hundreds of calls)

    def summary(bs):
        pooled = [x for blk in bs for x in blk]
        return dict(median_ms=round(statistics.median(pooled), 4), min_ms=round(min(pooled), 4),
                    block_median_ms=[round(statistics.median(blk), 4) for blk in bs])

    out = {k: summary(v) for k, v in blocks.items()}
    traffic = {"gs_mcmc_add_noise": 68 * n, "stream_copy_equal_traffic": 68 * n, "stream_copy_68n_bytes": 136 * n,
               "gs_mcmc_add_noise_rotating": 68 * n, "stream_copy_equal_traffic_rotating": 68 * n}
    for k, nbytes in traffic.items():
        out[k]["traffic_bytes"] = nbytes
        out[k]["gbs"] = round(nbytes / out[k]["median_ms"] / 1e6, 1)
    noise_ms = out["gs_mcmc_add_noise"]["median_ms"]
    out["noise_over_equal_traffic_copy"] = round(noise_ms / out["stream_copy_equal_traffic"]["median_ms"], 3)
    out["noise_over_copy_of_68n_bytes"] = round(noise_ms / out["stream_copy_68n_bytes"]["median_ms"], 3)
    out["noise_over_equal_traffic_copy_rotating"] = round(out["gs_mcmc_add_noise_rotating"]["median_ms"]
                                                          / out["stream_copy_equal_traffic_rotating"]["median_ms"], 3)
    out["pytorch_over_noise_kernel"] = round(out["pytorch_noise"]["median_ms"] / noise_ms, 2)
    out["pytorch_elementwise_over_noise_kernel"] = round(out["pytorch_noise_elementwise"]["median_ms"] / noise_ms, 2)
    out["relocate_1pc_dead"]["dead_rows"] = int(dead_rows.shape[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2_860_000, 100_000])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "mcmc_cost.json"))
    args = ap.parse_args()
    record = {"what": "events on the current stream, one process, alternating blocks per round and size: gs_mcmc_add_noise; "
                      "gs_stream_copy with the same traffic (34 N bytes copied) and of 68 N bytes; the first two over three sets "
                      "of buffers in turn (_rotating); the PyTorch composition "
                      "of the noise step with torch.bmm and with broadcast multiply-and-sum; one MCMCController.relocate() with 1 % dead rows on six tensors (widths 3, 4, 3, "
                      "1, 3, 45) with Adam moments, host read included",
              "rounds": args.rounds, "reps": args.reps, "sizes": {}}
    for n in args.n:
        if n % 8:
            raise SystemExit("--n must be a multiple of 8 (the stream copy moves 16-byte pieces)")
        r = record["sizes"][str(n)] = measure(n, args.rounds, args.reps)
        print(json.dumps({str(n): {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in r.items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(os.path.abspath(args.out), ROOT)}))


if __name__ == "__main__":
    main()
