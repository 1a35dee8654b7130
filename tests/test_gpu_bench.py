"""bench.py's plain run on the GPU: the line carries the contract's fields for exactly --steps timed steps and nothing
that only --full measures, and --dump-outputs writes what the timed path (fused.rasterize forward + backward) computes
for the bench's inputs -- the same frame computed here, in the test's own process, from the same seeded scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", "A", "--spinup-steps", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["ms_per_step"] > 0
    assert line["unit"] == "Mpixels/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - 256 * 256 / (line["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert line["other_workloads"] == {} and line["config"]["S"] is None

    from gaussian_splatting_amd import fused
    from gaussian_splatting_amd.synthetic import DEFAULTS, WORKLOADS, make_grad_image, make_scene
    N, W, H, deg = WORKLOADS["A"]
    dev = torch.device("cuda", 0)
    g, cam, T = make_scene(N, W, H, deg, seed=0, device=dev)
    names = [k for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh") if getattr(g, k) is not None]
    for k in names:
        getattr(g, k).requires_grad_(True)
    img, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=torch.zeros(3, device=dev),
                                    **DEFAULTS)
    img.backward(make_grad_image(W, H, seed=1, device=dev))

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sorted(got) == sorted(["image", "mask", "uv"] + [f"grad_{k}" for k in names])   # A: no row is sampled
    assert np.array_equal(got["image"], img.detach().cpu().numpy())
    assert np.array_equal(got["mask"], mask.cpu().float().numpy())
    assert np.array_equal(got["uv"], uv.detach().cpu().numpy())
    for k in names:
        ref = getattr(g, k).grad.cpu().double().numpy()
        err = np.abs(got[f"grad_{k}"] - ref).max() / max(np.abs(ref).max(), 1e-30)
        assert err < 1e-5, f"grad {k}: {err}"   # fp32 summation order of the gradient atomics
